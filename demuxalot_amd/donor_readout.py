"""Host side of the donor-level read-outs of DevicePosteriors (demux.py): the column <-> (g1, g2) mapping of the option
columns and the composition of per-droplet calls and per-donor summaries from the B-length arrays the device pass returns
(include/demux_hip_debug.h: dmx_get_donor_readout, dmx_get_allowed_mass).  Pure numpy / pandas: imports without a GPU.

Columns (demux.py: _option_names): singlets 0 .. G-1, then the pairs (g1 < g2) in the order of
`for g1 in range(G): for g2 in range(g1 + 1, G)`, i.e. pair (g1, g2) at G + g1 (2G - g1 - 1) / 2 + (g2 - g1 - 1)."""
import numpy as np
import pandas as pd


def n_options(n_donors, with_doublets):
    return n_donors * (n_donors + 1) // 2 if with_doublets else n_donors


def pair_column(n_donors, g1, g2):
    """Column of the pair (g1 < g2); arrays broadcast."""
    g1, g2 = np.asarray(g1, dtype=np.int64), np.asarray(g2, dtype=np.int64)
    assert ((0 <= g1) & (g1 < g2) & (g2 < n_donors)).all(), 'a pair is g1 < g2 < G'
    return n_donors + g1 * (2 * n_donors - g1 - 1) // 2 + (g2 - g1 - 1)


def pair_first_columns(n_donors):
    """int64[G]: the column of (g1, g1 + 1) for every g1 - where the pairs that start with g1 begin (the last entry is K)."""
    g1 = np.arange(n_donors, dtype=np.int64)
    return n_donors + g1 * (2 * n_donors - g1 - 1) // 2


def column_donors(n_donors, columns):
    """(g1, g2) of option columns, int64 arrays: a singlet column g gives (g, -1), a negative column (-1: none) gives (-1, -1)."""
    columns = np.asarray(columns, dtype=np.int64)
    assert (columns < n_options(n_donors, True)).all(), 'column beyond the pairs of the donors'
    first = pair_first_columns(n_donors)
    is_pair = columns >= n_donors
    g1 = np.searchsorted(first, columns, side='right') - 1  # the last g1 whose pairs begin at or before the column
    g1 = np.where(is_pair, g1, columns)
    g2 = np.where(is_pair, columns - first[np.clip(g1, 0, max(n_donors - 1, 0))] + g1 + 1, -1)
    g1 = np.where(columns < 0, -1, g1)
    return g1, np.where(columns < 0, -1, g2)


def donor_columns(n_donors, donor, with_doublets):
    """The columns of the options that contain `donor`, ascending: its singlet, (0, g) .. (g-1, g), (g, g+1) .. (g, G-1)."""
    if not with_doublets:
        return np.array([donor], dtype=np.int64)
    before = np.arange(donor, dtype=np.int64)
    after = np.arange(donor + 1, n_donors, dtype=np.int64)
    return np.concatenate([[donor], pair_column(n_donors, before, donor), pair_column(n_donors, donor, after)]).astype(np.int64)


def compose_calls(donor_names, threshold, best_singlet, best_singlet_prob, best_pair, doublet_mass, index=None):
    """DevicePosteriors.droplet_calls from the device pass's arrays.  Per droplet, in this order of precedence:
      'singlet'     best singlet posterior > threshold, compared in float32 as DevicePosteriors.assignments compares
                    (Series.gt on a float32 column): donor_1 is that donor, probability the posterior;
      'doublet'     doublet_mass > threshold, compared in float64: donor_1, donor_2 are the donors of the best pair column,
                    probability is doublet_mass;
      'unassigned'  otherwise: no donors, probability is the larger of the two (NaN counts as absent)."""
    G = len(donor_names)
    best_singlet, best_pair = np.asarray(best_singlet, dtype=np.int64), np.asarray(best_pair, dtype=np.int64)
    best_singlet_prob = np.asarray(best_singlet_prob, dtype=np.float32)
    doublet_mass = np.asarray(doublet_mass, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        singlet = (best_singlet >= 0) & (best_singlet_prob > np.float32(threshold))
        doublet = ~singlet & (best_pair >= 0) & (doublet_mass > np.float64(threshold))
    names = np.asarray(list(donor_names) + [None], dtype=object)  # -1 -> None
    p1, p2 = column_donors(G, best_pair)
    donor_1 = np.where(singlet, names[np.where(singlet, best_singlet, -1)], names[np.where(doublet, p1, -1)])
    donor_2 = names[np.where(doublet, p2, -1)]
    status = np.where(singlet, 'singlet', np.where(doublet, 'doublet', 'unassigned')).astype(object)
    singlet_p = best_singlet_prob.astype(np.float64)
    probability = np.where(singlet, singlet_p, np.where(doublet, doublet_mass, np.fmax(singlet_p, doublet_mass)))
    return pd.DataFrame({'status': status, 'donor_1': donor_1, 'donor_2': donor_2, 'probability': probability,
                         'doublet_probability': doublet_mass}, index=index)


def expected_cells(n_donors, option_sums):
    """float64[G]: a donor's own column sum plus those of its pair columns, added in ascending column order - the column sums of
    the donor marginals, from the K option sums alone."""
    option_sums = np.asarray(option_sums, dtype=np.float64)
    assert len(option_sums) in (n_donors, n_options(n_donors, True)), 'option sums of another shape'
    with_doublets = len(option_sums) != n_donors
    out = np.zeros(n_donors, dtype=np.float64)
    for g in range(n_donors):
        for k in donor_columns(n_donors, g, with_doublets):
            out[g] += option_sums[k]
    return out


def compose_summary(donor_names, calls, option_sums):
    """DevicePosteriors.donor_summary from droplet_calls' frame and the option sums: per donor n_singlets, n_doublets (droplets
    called doublet whose best pair contains the donor) and expected_cells."""
    names = list(donor_names)
    position = {name: g for g, name in enumerate(names)}
    n_singlets, n_doublets = np.zeros(len(names), dtype=np.int64), np.zeros(len(names), dtype=np.int64)
    status = calls['status'].values
    for which, column, counts in (('singlet', 'donor_1', n_singlets), ('doublet', 'donor_1', n_doublets), ('doublet', 'donor_2', n_doublets)):
        donors = calls[column].values[status == which]
        np.add.at(counts, np.fromiter((position[d] for d in donors), dtype=np.int64, count=len(donors)), 1)
    return pd.DataFrame({'n_singlets': n_singlets, 'n_doublets': n_doublets, 'expected_cells': expected_cells(len(names), option_sums)},
                        index=pd.Index(names, name='donor'))


def allowed_lists(barcodes, columns, barcode2possible_options):
    """CSR (start int64[B + 1], options int32) of the option columns possible for each barcode, in the order the dict lists
    them.  ValueError where the reference's _compute_qualities asserts (utils.py:273, 279): a barcode that is not in the dict, a
    name (anywhere in the dict) that is not a column."""
    position = {name: k for k, name in enumerate(columns)}
    for barcode, options in barcode2possible_options.items():
        unknown = [o for o in options if o not in position]
        if unknown:
            raise ValueError(f'some of the options of {barcode!r} are not columns of the posteriors: {unknown}')
    start = np.zeros(len(barcodes) + 1, dtype=np.int64)
    flat = []
    for b, barcode in enumerate(barcodes):
        if barcode not in barcode2possible_options:
            raise ValueError(f'barcode {barcode!r} is not in barcode2possible_options')
        flat.extend(position[o] for o in barcode2possible_options[barcode])
        start[b + 1] = len(flat)
    return start, np.asarray(flat, dtype=np.int32)


def compose_qualities(mass, best_is_allowed):
    """The reference's metrics (utils.py:288-296) from the device pass's float64 masses: logloss = mean(-log(max(mass, 1e-4)))."""
    mass = np.asarray(mass, dtype=np.float64)
    accuracy = np.mean(np.asarray(best_is_allowed) != 0)
    return {'logloss': np.mean(-np.log(np.maximum(mass, 1e-4))), 'accuracy': accuracy, 'error rate': 1 - accuracy}
