"""Plain numpy / pandas restatement of the donor-level read-outs (include/demux_hip_debug.h: dmx_get_donor_readout,
dmx_get_allowed_mass; DevicePosteriors.droplet_calls / donor_summary / qualities), used as the checker by
tests/test_donor_readout_cpu.py and tests/test_gpu_donor_readout.py.  Written from the contract, not from the implementation:
the columns are enumerated the way demux.py's _option_names enumerates their names."""
import numpy as np
import pandas as pd


def enumerate_options(G, with_doublets):
    """[(g,) or (g1, g2)] per column: singlets, then `for g1: for g2 > g1`."""
    options = [(g,) for g in range(G)]
    if with_doublets:
        options += [(g1, g2) for g1 in range(G) for g2 in range(g1 + 1, G)]
    return options


def readout(P, G):
    """dict of the arrays dmx_get_donor_readout returns for float32 posteriors P [B, K]."""
    P = np.asarray(P)
    assert P.dtype == np.float32
    B, K = P.shape
    with_doublets = K != G
    options = enumerate_options(G, with_doublets)
    assert len(options) == K
    singlets, pairs = P[:, :G], P[:, G:]
    out = dict(singlet_mass=singlets.astype(np.float64).sum(axis=1), doublet_mass=pairs.astype(np.float64).sum(axis=1))
    out['best_singlet'] = np.argmax(singlets, axis=1).astype(np.int32) if B else np.zeros(0, np.int32)
    out['best_singlet_prob'] = singlets[np.arange(B), out['best_singlet']]
    if K > G:
        out['best_pair'] = (G + np.argmax(pairs, axis=1)).astype(np.int32) if B else np.zeros(0, np.int32)
        out['best_pair_prob'] = P[np.arange(B), out['best_pair']]
    else:
        out['best_pair'] = np.full(B, -1, dtype=np.int32)
        out['best_pair_prob'] = np.full(B, np.nan, dtype=np.float32)
    marginals = np.zeros((B, G), dtype=np.float32)
    for g in range(G):
        total = np.zeros(B, dtype=np.float64)
        for k, option in enumerate(options):  # ascending column order, one float64 addition per column
            if g in option:
                total = total + P[:, k].astype(np.float64)
        marginals[:, g] = total.astype(np.float32)  # rounded once
    out['donor_marginals'] = marginals
    return out


def allowed_mass(P, start, options):
    """(mass float64[B], best_is_allowed int32[B]): sequential float64 sums in list order; the row's first maximum listed?"""
    P = np.asarray(P)
    B = len(P)
    mass, hit = np.zeros(B, dtype=np.float64), np.zeros(B, dtype=np.int32)
    for b in range(B):
        listed = [int(k) for k in options[start[b]:start[b + 1]]]
        total = np.float64(0)
        for k in listed:
            total = total + np.float64(P[b, k])
        mass[b] = total
        hit[b] = int(np.argmax(P[b])) in listed
    return mass, hit


def calls(P, donor_names, threshold):
    """DevicePosteriors.droplet_calls for the posteriors P whose first len(donor_names) columns are the singlets."""
    G = len(donor_names)
    P = np.asarray(P)
    options = enumerate_options(G, P.shape[1] != G)
    rows = []
    for row in P:
        best = int(np.argmax(row[:G]))
        doublet_mass = np.float64(row[G:].astype(np.float64).sum())
        if row[best] > np.float32(threshold):
            rows.append(('singlet', donor_names[best], None, np.float64(row[best]), doublet_mass))
        elif len(row) > G and doublet_mass > threshold:
            g1, g2 = options[G + int(np.argmax(row[G:]))]
            rows.append(('doublet', donor_names[g1], donor_names[g2], doublet_mass, doublet_mass))
        else:
            rows.append(('unassigned', None, None, max(np.float64(row[best]), doublet_mass), doublet_mass))
    return pd.DataFrame(rows, columns=['status', 'donor_1', 'donor_2', 'probability', 'doublet_probability'])


def summary(P, donor_names, threshold):
    """DevicePosteriors.donor_summary: counts from calls(), expected_cells as the float64 column sums of the marginals' terms."""
    G = len(donor_names)
    P = np.asarray(P)
    frame = calls(P, donor_names, threshold)
    options = enumerate_options(G, P.shape[1] != G)
    sums = P.astype(np.float64).sum(axis=0)
    out = pd.DataFrame({'n_singlets': 0, 'n_doublets': 0, 'expected_cells': 0.0}, index=pd.Index(list(donor_names), name='donor'))
    for g, name in enumerate(donor_names):
        out.loc[name, 'n_singlets'] = int(((frame['status'] == 'singlet') & (frame['donor_1'] == name)).sum())
        out.loc[name, 'n_doublets'] = int(((frame['status'] == 'doublet') & ((frame['donor_1'] == name) | (frame['donor_2'] == name))).sum())
        out.loc[name, 'expected_cells'] = sum(sums[k] for k, option in enumerate(options) if g in option)
    return out


def qualities_float64(probs_df, barcode2possible_options):
    """logloss = mean(-log(max(p, 1e-4))), p the float64 sum (in list order) of the posteriors of the barcode's possible options;
    accuracy = share of barcodes whose first most probable option is possible; error rate = 1 - accuracy."""
    columns = list(probs_df.columns)
    losses, correct = [], []
    for barcode, row in zip(probs_df.index, probs_df.values):
        possible = barcode2possible_options[barcode]
        p = np.float64(0)
        for name in possible:
            p = p + np.float64(row[columns.index(name)])
        losses.append(-np.log(max(p, 1e-4)))
        correct.append(columns[int(np.argmax(row))] in possible)
    return {'logloss': np.mean(losses), 'accuracy': np.mean(correct), 'error rate': 1 - np.mean(correct)}


def qualities_pandas_float32(probs_df, barcode2possible_options):
    """The same in pandas on the float32 frame, as the reference evaluates it: a float32 Series sum, clipped below at 1e-4,
    a float32 log; idxmax for the most probable option."""
    losses, correct = [], []
    for barcode, row in probs_df.iterrows():
        possible = barcode2possible_options[barcode]
        p = row[possible].sum()
        losses.append(-np.log(p.clip(1e-4)))
        correct.append(row.idxmax() in possible)
    return {'logloss': np.mean(losses), 'accuracy': np.mean(correct), 'error rate': 1 - np.mean(correct)}
