"""Per-barcode ambient RNA fractions (Demultiplexer.estimate_ambient).

How much of a droplet's signal is NOT from the option it was assigned to: for every barcode the log-likelihood of its calls when a
share alpha of its molecules comes from the soup, on a grid of alphas; the estimate is the grid value of the first maximum.  The
device pass (include/demux_hip_debug.h: dmx_ambient_profile) returns B-length read-outs and, if asked, the [B, A] profile; this
module resolves the caller's assignments into table columns and composes the frames.  JointAmbientPosteriors is the result of
Demultiplexer.predict_posteriors_joint_ambient: every option scored at its own best fraction of the grid.  Pure
numpy / pandas: imports without a GPU.
"""
import numbers

import numpy as np
import pandas as pd

from . import donor_readout


def default_alphas():
    """The grid of estimate_ambient: 64 values, 0 .. 0.63 in steps of 0.01, one per lane of the device pass."""
    return np.linspace(0, 0.63, 64, dtype=np.float32)


def _is_skip(value):
    if value is None:
        return True
    if isinstance(value, (float, np.floating)) and np.isnan(value):
        return True
    return isinstance(value, (numbers.Integral, np.integer)) and not isinstance(value, (bool, np.bool_)) and int(value) == -1


def resolve_assignments(option_names, ordered_barcodes, assignments):
    """int64[B] option columns (-1: skip) from a Series or mapping barcode -> option name | integer option column | None / NaN / -1.
    option_names: the columns of the posteriors (singlets, then 'A+B'); a name is looked up exactly, never split on '+', so donor
    names may contain one.  A barcode of the handler that `assignments` does not mention is skipped.  ValueError: a name that is no
    option, a column outside the options, a barcode that is not the handler's."""
    column_of = {}
    for k, name in enumerate(option_names):
        column_of.setdefault(name, k)  # (the first of equal names, as an exact look-up of the frame's columns would find)
    row_of = {barcode: b for b, barcode in enumerate(ordered_barcodes)}
    columns = np.full(len(ordered_barcodes), -1, dtype=np.int64)
    items = assignments.items() if hasattr(assignments, 'items') else dict(assignments).items()
    for barcode, value in items:
        if barcode not in row_of:
            raise ValueError(f'assignments: barcode {barcode!r} is not one of the barcode handler')
        if _is_skip(value):
            continue
        if isinstance(value, (numbers.Integral, np.integer)) and not isinstance(value, (bool, np.bool_)):
            if not 0 <= int(value) < len(option_names):
                raise ValueError(f'assignments: option column {int(value)} of barcode {barcode!r} is outside [0, {len(option_names)})')
            columns[row_of[barcode]] = int(value)
        elif value in column_of:
            columns[row_of[barcode]] = column_of[value]
        else:
            raise ValueError(f'assignments: {value!r} of barcode {barcode!r} is not an option')
    return columns


def resolve_fractions(ordered_barcodes, ambient_fractions):
    """float32[B] per-barcode fractions (predict_posteriors_with_ambient) from a Series or mapping barcode -> alpha.  A barcode that
    is missing, None or NaN gets 0: it is scored as predict_posteriors scores it.  ValueError: a value that is no number or lies
    outside [0, 1] (as float32, which is what the device pass reads), a barcode that is not the handler's."""
    row_of = {barcode: b for b, barcode in enumerate(ordered_barcodes)}
    alpha = np.zeros(len(ordered_barcodes), dtype=np.float32)
    items = ambient_fractions.items() if hasattr(ambient_fractions, 'items') else dict(ambient_fractions).items()
    for barcode, value in items:
        if barcode not in row_of:
            raise ValueError(f'ambient_fractions: barcode {barcode!r} is not one of the barcode handler')
        if value is None:
            continue
        if isinstance(value, (bool, np.bool_)) or not isinstance(value, (numbers.Real, np.number)):
            raise ValueError(f'ambient_fractions: {value!r} of barcode {barcode!r} is not a number')
        if np.isnan(value):
            continue
        as_f32 = np.float32(value)
        if not (0 <= value <= 1 and np.float32(0) <= as_f32 <= np.float32(1)):
            raise ValueError(f'ambient_fractions: {value!r} of barcode {barcode!r} is outside [0, 1]')
        alpha[row_of[barcode]] = as_f32
    return alpha


def best_singlets(logits, n_donors):
    """int64[B]: every barcode's best singlet - the first maximum over the first n_donors columns of the plain logits (the singlets'
    penalty is 0: these are the donors' log-likelihoods), whatever the doublet columns say; -1 where every singlet logit is NaN."""
    singlets = np.asarray(logits)[:, :n_donors]
    nan = np.isnan(singlets)
    first = np.where(nan, -np.inf, singlets).argmax(axis=1)
    return np.where(nan.all(axis=1), -1, first).astype(np.int64)


def assigned_donors(n_donors, columns):
    """(donor1, donor2) int32[B] as the device pass takes them: table columns, (-1, -1) skipped, (d, -1) a singlet, d1 < d2 a pair."""
    d1, d2 = donor_readout.column_donors(n_donors, columns)
    return d1.astype(np.int32), d2.astype(np.int32)


def resolve_grid(alphas):
    """float32[A] grid of predict_posteriors_joint_ambient: None -> default_alphas(); otherwise the values as float32, one-dimensional.
    ValueError: an empty grid, more than 64 values, a value that is not finite or lies outside [0, 1] (as float32, which is what
    the device pass reads)."""
    if alphas is None:
        return default_alphas()
    grid = np.ascontiguousarray(alphas, dtype=np.float32).reshape(-1)
    if not 1 <= len(grid) <= 64:
        raise ValueError(f'alphas: the grid has {len(grid)} values; 1 .. 64 are supported')
    if not ((grid >= 0) & (grid <= 1)).all():  # (NaN fails both)
        raise ValueError('alphas: a grid value is not finite or outside [0, 1]')
    return grid


class JointAmbientPosteriors:
    """The result of one predict_posteriors_joint_ambient call, host-resident: every option - singlets and pairs - scored at its own
    best ambient fraction of the grid, one softmax over those scores.

    posteriors: (logits_df, probs_df) with predict_posteriors' index and columns, or, for a call with pools, a PooledPosteriors;
    alphas float32[A]: the grid; ambient float32[V]: the soup's allele profile that was used; row_ptr int64[B + 1]: barcode b owns the
    entries row_ptr[b] .. row_ptr[b + 1] of the compact per-option arrays; alpha_index int32[row_ptr[B]]: the grid point of every
    option's first maximum (-1: every value NaN); option_alphas float64[row_ptr[B]]: its grid value, NaN where there is none;
    best_option, best_prob, doublet_mass, best_alpha_index [B]: the read-outs of the pass (-1 / NaN / NaN / -1 for a barcode in no
    pool); profile float32[row_ptr[B], A]: every option's logit at every grid point, or None when it was not kept.
    over_grid: 'max', or 'marginal' - every option's logit the log of the (weighted) sum over the grid, alpha_index the grid point of
    the largest term; then option_alpha_means float64[row_ptr[B]] is every option's posterior mean fraction (NaN where there is
    none) and best_alpha_mean float32[B] that of best_option; under 'max' both are None."""

    def __init__(self, barcodes, option_names, pool_of_barcode, row_ptr, alphas, ambient, alpha_index, best_option, best_prob, doublet_mass,
                 best_alpha_index, posteriors, profile=None, index_name='BARCODE', over_grid='max', alpha_mean=None, best_alpha_mean=None):
        self.barcodes = list(barcodes)
        self._option_names = [list(names) for names in option_names]  # per pool
        self.pool_of_barcode = np.asarray(pool_of_barcode, dtype=np.int32)
        self.row_ptr = np.asarray(row_ptr, dtype=np.int64)
        self.alphas = np.asarray(alphas, dtype=np.float32)
        self.ambient = np.asarray(ambient, dtype=np.float32)
        self.alpha_index = np.asarray(alpha_index, dtype=np.int32)
        self.best_option = np.asarray(best_option, dtype=np.int32)
        self.best_prob = np.asarray(best_prob, dtype=np.float32)
        self.doublet_mass = np.asarray(doublet_mass, dtype=np.float64)
        self.best_alpha_index = np.asarray(best_alpha_index, dtype=np.int32)
        self.posteriors = posteriors
        self.index_name = index_name
        B = len(self.barcodes)
        n = int(self.row_ptr[-1]) if B else 0
        assert self.pool_of_barcode.shape == (B,) and self.row_ptr.shape == (B + 1,) and self.alpha_index.shape == (n,)
        assert self.best_option.shape == (B,) and self.best_prob.shape == (B,) and self.doublet_mass.shape == (B,) and self.best_alpha_index.shape == (B,)
        widths = np.array([len(names) for names in self._option_names] + [0], dtype=np.int64)  # (-1 -> no entries)
        assert np.array_equal(np.diff(self.row_ptr), widths[self.pool_of_barcode]), 'row_ptr does not follow the pools'
        assert ((self.alpha_index >= -1) & (self.alpha_index < len(self.alphas))).all()
        self.option_alphas = self._grid_values(self.alpha_index)
        assert over_grid in ('max', 'marginal') and (over_grid == 'marginal') == (alpha_mean is not None) == (best_alpha_mean is not None)
        self.over_grid = over_grid
        self.option_alpha_means = self.best_alpha_mean = None
        if over_grid == 'marginal':
            self.option_alpha_means = np.asarray(alpha_mean, dtype=np.float32).astype(np.float64)
            self.best_alpha_mean = np.asarray(best_alpha_mean, dtype=np.float32)
            assert self.option_alpha_means.shape == self.option_alphas.shape and self.best_alpha_mean.shape == (B,)
        self.profile = None
        if profile is not None:
            self.profile = np.asarray(profile, dtype=np.float32)
            assert self.profile.shape == (n, len(self.alphas))

    def _grid_values(self, index):
        found = index >= 0
        return np.where(found, self.alphas[np.where(found, index, 0)].astype(np.float64), np.nan)

    def _index(self):
        index = pd.Index(self.barcodes)
        index.name = self.index_name
        return index

    def alphas_of(self, barcode) -> pd.Series:
        """option name -> the grid value of that option's maximum, for one barcode (empty for a barcode in no pool)."""
        b = self.barcodes.index(barcode)
        p = self.pool_of_barcode[b]
        names = self._option_names[p] if p >= 0 else []
        return pd.Series(self.option_alphas[self.row_ptr[b]:self.row_ptr[b + 1]], index=names, name='alpha')

    def summary(self) -> pd.DataFrame:
        """Per barcode (all of them, handler order): `option`, the name of the most probable option (None: none, or in no pool);
        `probability`, its posterior; `alpha`, the grid value at which that option was scored (NaN: none); `doublet_probability`,
        the posterior mass of the pair options (float64); `at_grid_edge`: that alpha is the largest grid value, so the maximum may
        lie beyond the grid.  Under over_grid='marginal' `alpha` is the grid value of that option's largest term, and one more
        column, `alpha_mean`, holds its posterior mean fraction (float64; NaN: none)."""
        option = np.empty(len(self.barcodes), dtype=object)
        for b, (p, k) in enumerate(zip(self.pool_of_barcode, self.best_option)):
            option[b] = self._option_names[p][k] if p >= 0 and k >= 0 else None
        alpha = self._grid_values(self.best_alpha_index)
        at_edge = (self.best_alpha_index >= 0) & (alpha == np.float64(self.alphas.max()))
        frame = pd.DataFrame({'option': option, 'probability': self.best_prob, 'alpha': alpha, 'doublet_probability': self.doublet_mass,
                              'at_grid_edge': at_edge}, index=self._index())
        if self.over_grid == 'marginal':
            frame['alpha_mean'] = self.best_alpha_mean.astype(np.float64)
        return frame


class DeviceJointAmbientPosteriors:
    """The result of one predict_posteriors_joint_ambient call with on_device=True: the compact rows - logits, posteriors, every
    option's grid point and, under 'marginal', its posterior mean fraction - stay on the GPU; what is held here is
    B-sized.  posteriors: the DevicePooledPosteriors of the call (without pools: one pool, 'all'); alphas, ambient, over_grid,
    best_alpha_index and best_alpha_mean as JointAmbientPosteriors holds them.  close() closes the posteriors."""

    def __init__(self, posteriors, alphas, ambient, best_alpha_index, over_grid='max', best_alpha_mean=None):
        self.posteriors = posteriors
        self.barcodes = posteriors.barcodes
        self.alphas = np.asarray(alphas, dtype=np.float32)
        self.ambient = np.asarray(ambient, dtype=np.float32)
        self.best_alpha_index = np.asarray(best_alpha_index, dtype=np.int32)
        assert over_grid in ('max', 'marginal') and (over_grid == 'marginal') == (best_alpha_mean is not None)
        self.over_grid = over_grid
        self.best_alpha_mean = None if best_alpha_mean is None else np.asarray(best_alpha_mean, dtype=np.float32)
        assert self.best_alpha_index.shape == (len(self.barcodes),)

    def _grid_values(self, index):
        found = index >= 0
        return np.where(found, self.alphas[np.where(found, index, 0)].astype(np.float64), np.nan)

    def _row(self, barcode, what):
        post = self.posteriors
        b = post.barcodes.index(barcode)
        p = post.pool_of_barcode[b]
        names = post.columns_of(post.pools[p]) if p >= 0 else []
        return post._ctx.pooled_get(what, b, b + 1, len(names)), names

    def alphas_of(self, barcode) -> pd.Series:
        """option name -> the grid value of that option's maximum, for one barcode (empty for a barcode in no pool): one row of
        the resident alpha_index."""
        index, names = self._row(barcode, 'alpha_index')
        return pd.Series(self._grid_values(index), index=names, name='alpha')

    def alpha_means_of(self, barcode) -> pd.Series:
        """('marginal' only) option name -> that option's posterior mean fraction, for one barcode."""
        if self.over_grid != 'marginal':
            raise ValueError("posterior mean fractions come with over_grid='marginal'")
        mean, names = self._row(barcode, 'alpha_mean')
        return pd.Series(mean.astype(np.float64), index=names, name='alpha_mean')

    def summary(self) -> pd.DataFrame:
        """JointAmbientPosteriors.summary(), from the B-sized read-outs alone."""
        post = self.posteriors
        alpha = self._grid_values(self.best_alpha_index)
        at_edge = (self.best_alpha_index >= 0) & (alpha == np.float64(self.alphas.max()))
        frame = pd.DataFrame({'option': post._option_labels(post.best_option), 'probability': post.best_prob, 'alpha': alpha,
                              'doublet_probability': post.doublet_mass, 'at_grid_edge': at_edge}, index=post._index())
        if self.over_grid == 'marginal':
            frame['alpha_mean'] = self.best_alpha_mean.astype(np.float64)
        return frame

    def close(self):
        self.posteriors.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class AmbientEstimate:
    """The result of one estimate_ambient call, host-resident.

    alphas float32[A]: the grid; ambient float32[V]: the soup's allele profile that was used; profile: DataFrame [B, A] of the
    log-likelihoods (columns: the grid values), or None when it was not kept; best int32[B]: the grid point of the first maximum
    (-1: skipped); ll_best / ll_zero float32[B]: the log-likelihood there and at the first alpha == 0 (NaN: skipped / no 0 on the
    grid)."""

    def __init__(self, barcodes, option_names, columns, alphas, ambient, best, ll_best, ll_zero, loglik=None, index_name='BARCODE'):
        self.barcodes = list(barcodes)
        self.alphas = np.asarray(alphas, dtype=np.float32)
        self.ambient = np.asarray(ambient, dtype=np.float32)
        self.best = np.asarray(best, dtype=np.int32)
        self.ll_best = np.asarray(ll_best, dtype=np.float32)
        self.ll_zero = np.asarray(ll_zero, dtype=np.float32)
        self.index_name = index_name
        self._option_names = list(option_names)
        self._columns = np.asarray(columns, dtype=np.int64)
        B = len(self.barcodes)
        assert self._columns.shape == (B,) and self.best.shape == (B,) and self.ll_best.shape == (B,) and self.ll_zero.shape == (B,)
        self.profile = None
        if loglik is not None:
            loglik = np.asarray(loglik, dtype=np.float32)
            assert loglik.shape == (B, len(self.alphas))
            self.profile = pd.DataFrame(loglik, index=self._index(), columns=self.alphas)

    def _index(self):
        index = pd.Index(self.barcodes)
        index.name = self.index_name
        return index

    def fractions(self) -> pd.Series:
        """barcode -> the estimated alpha (float64: the grid value of the first maximum), NaN where the barcode was skipped; all
        barcodes, handler order.  What predict_posteriors_with_ambient takes as `ambient_fractions`."""
        found = self.best >= 0
        alpha = np.where(found, self.alphas[np.where(found, self.best, 0)].astype(np.float64), np.nan)
        return pd.Series(alpha, index=self._index(), name='alpha')

    def summary(self) -> pd.DataFrame:
        """Per barcode (all of them, handler order): `option`, the name it was assigned (None: skipped); `alpha`, the grid value of
        the first maximum (NaN: skipped); `log_likelihood_ratio`, float64 ll_best - ll_zero (how much better the estimate explains
        the calls than no contamination; NaN where the grid has no 0); `at_grid_edge`: the estimate is the largest grid value, so
        the maximum may lie beyond the grid."""
        names = np.asarray(self._option_names + [None], dtype=object)
        found = self.best >= 0
        alpha = np.where(found, self.alphas[np.where(found, self.best, 0)].astype(np.float64), np.nan)
        ratio = self.ll_best.astype(np.float64) - self.ll_zero.astype(np.float64)
        at_edge = found & (alpha == np.float64(self.alphas.max()))
        return pd.DataFrame({'option': names[self._columns], 'alpha': alpha, 'log_likelihood_ratio': ratio, 'at_grid_edge': at_edge},
                            index=self._index())
