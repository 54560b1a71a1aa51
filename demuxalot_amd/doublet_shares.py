"""Doublets of unequal shares (Demultiplexer.predict_posteriors_with_doublet_shares; include/demux_hip_debug.h: dmx_estep_pair_shares;
DESIGN.md 4.12): the grid of mixing shares and the host-resident result of the pass."""
import numpy as np
import pandas as pd


def default_shares():
    """0.1, 0.2 .. 0.9 as float32: the share of a pair's first-named donor."""
    return (np.arange(1, 10, dtype=np.float64) / 10).astype(np.float32)


def resolve_shares(shares, share_log_weights):
    """(float32[n] grid, float32[n] log weights) of predict_posteriors_with_doublet_shares.  shares None -> default_shares();
    share_log_weights None -> the uniform prior, float32(-log(n)) per point.  ValueError: an empty grid, more than 64 values, a share
    that is not finite or lies outside [0, 1] (as float32, which is what the device pass reads), weights that are not one finite value
    per share."""
    grid = default_shares() if shares is None else np.ascontiguousarray(shares, dtype=np.float32).reshape(-1)
    if not 1 <= len(grid) <= 64:
        raise ValueError(f'shares: the grid has {len(grid)} values; 1 .. 64 are supported')
    if not ((grid >= 0) & (grid <= 1)).all():  # (NaN fails both)
        raise ValueError('shares: a share is not finite or outside [0, 1]')
    if share_log_weights is None:
        weights = np.full(len(grid), np.float32(-np.log(len(grid))), dtype=np.float32)
    else:
        weights = np.ascontiguousarray(share_log_weights, dtype=np.float32).reshape(-1)
        if weights.shape != grid.shape or not np.isfinite(weights).all():
            raise ValueError('share_log_weights: one finite value per share')
    return grid, weights


class DoubletSharePosteriors:
    """The result of one predict_posteriors_with_doublet_shares call, host-resident: every pair option scored as the marginal over a
    grid of mixing shares, singlet options as predict_posteriors scores them, one softmax over those.

    posteriors: (logits_df, probs_df) with predict_posteriors' index and columns, or, for a call with pools, a PooledPosteriors;
    shares float32[n]: the grid; log_weights float32[n]: the log of the prior over it that was used; row_ptr int64[B + 1]: barcode b
    owns the entries row_ptr[b] .. row_ptr[b + 1] of the compact per-option arrays; option_shares float64[row_ptr[B]]: for a pair
    'A+B' the posterior mean share of A, its first-named donor, NaN for a singlet; option_share_index int32[row_ptr[B]]: the grid point
    of a pair's largest term, -1 for a singlet; best_option, best_prob, doublet_mass, best_share_index, best_share_mean [B]: the
    read-outs of the pass (-1 / NaN / NaN / -1 / NaN for a barcode in no pool; the last two also where the best option is a singlet)."""

    def __init__(self, barcodes, option_names, pool_donor_names, pool_of_barcode, row_ptr, shares, log_weights, share_index, share_mean,
                 best_option, best_prob, doublet_mass, best_share_index, best_share_mean, posteriors, index_name='BARCODE'):
        self.barcodes = list(barcodes)
        self._option_names = [list(names) for names in option_names]  # per pool
        self._donor_names = [list(names) for names in pool_donor_names]
        self.pool_of_barcode = np.asarray(pool_of_barcode, dtype=np.int32)
        self.row_ptr = np.asarray(row_ptr, dtype=np.int64)
        self.shares = np.asarray(shares, dtype=np.float32)
        self.log_weights = np.asarray(log_weights, dtype=np.float32)
        self.option_share_index = np.asarray(share_index, dtype=np.int32)
        self.option_shares = np.asarray(share_mean, dtype=np.float32).astype(np.float64)
        self.best_option = np.asarray(best_option, dtype=np.int32)
        self.best_prob = np.asarray(best_prob, dtype=np.float32)
        self.doublet_mass = np.asarray(doublet_mass, dtype=np.float64)
        self.best_share_index = np.asarray(best_share_index, dtype=np.int32)
        self.best_share_mean = np.asarray(best_share_mean, dtype=np.float32)
        self.posteriors = posteriors
        self.index_name = index_name
        B = len(self.barcodes)
        n = int(self.row_ptr[-1]) if B else 0
        assert self.pool_of_barcode.shape == (B,) and self.row_ptr.shape == (B + 1,)
        assert self.option_share_index.shape == (n,) and self.option_shares.shape == (n,) and self.log_weights.shape == self.shares.shape
        for values in (self.best_option, self.best_prob, self.doublet_mass, self.best_share_index, self.best_share_mean):
            assert values.shape == (B,)
        widths = np.array([len(names) for names in self._option_names] + [0], dtype=np.int64)  # (-1 -> no entries)
        assert np.array_equal(np.diff(self.row_ptr), widths[self.pool_of_barcode]), 'row_ptr does not follow the pools'
        assert ((self.option_share_index >= -1) & (self.option_share_index < len(self.shares))).all()

    def _index(self):
        index = pd.Index(self.barcodes)
        index.name = self.index_name
        return index

    def _pair_donors(self, pool, option):
        """(first, second) donor names of a pair option of a pool, in the reference's order: the pairs i < j, i-major, behind the singlets."""
        donors = self._donor_names[pool]
        g, rest = len(donors), option - len(donors)
        for i in range(g):
            if rest < g - 1 - i:
                return donors[i], donors[i + 1 + rest]
            rest -= g - 1 - i
        raise IndexError(option)

    def shares_of(self, barcode) -> pd.Series:
        """option name -> the posterior mean share of the option's first-named donor (NaN: a singlet), for one barcode (empty for a
        barcode in no pool)."""
        b = self.barcodes.index(barcode)
        p = self.pool_of_barcode[b]
        names = self._option_names[p] if p >= 0 else []
        return pd.Series(self.option_shares[self.row_ptr[b]:self.row_ptr[b + 1]], index=names, name='share')

    def summary(self) -> pd.DataFrame:
        """Per barcode (all of them, handler order): `option`, the name of the most probable option (None: none, or in no pool);
        `probability`, its posterior; `doublet_probability`, the posterior mass of the pair options (float64); `share`, for a best
        option 'A+B' the posterior mean share of A (float64; NaN: a singlet or none); `major_donor`, the donor of that pair that
        holds the larger part - A at a share of 0.5 or more, else B (None: a singlet or none)."""
        option = np.empty(len(self.barcodes), dtype=object)
        major = np.empty(len(self.barcodes), dtype=object)
        share = self.best_share_mean.astype(np.float64)
        for b, (p, k) in enumerate(zip(self.pool_of_barcode, self.best_option)):
            option[b] = self._option_names[p][k] if p >= 0 and k >= 0 else None
            major[b] = None
            if p >= 0 and k >= len(self._donor_names[p]) and not np.isnan(share[b]):
                first, second = self._pair_donors(p, int(k))
                major[b] = first if share[b] >= 0.5 else second
        return pd.DataFrame({'option': option, 'probability': self.best_prob, 'doublet_probability': self.doublet_mass, 'share': share,
                             'major_donor': major}, index=self._index())
