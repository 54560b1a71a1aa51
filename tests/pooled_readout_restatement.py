"""Plain numpy restatement of the read-outs over a resident pooled result (include/demux_hip_debug.h: dmx_pooled_readout,
dmx_pooled_top_options, dmx_pooled_option_sums, dmx_pooled_allowed_mass; DevicePooledPosteriors), used as the checker by
tests/test_pooled_readout_cpu.py and tests/test_gpu_pooled_readout.py.  Written from the contract, not from the kernels: every sum is
a Python loop of float64 additions in the order the contract names, every maximum a scan that a NaN never wins.

A result is compact: barcode b of pool p = pool_of[b] owns probs[row_ptr[b]:row_ptr[b + 1]], the options of its pool in pool-local
order - the g_p singlets, then the pairs `for i: for j > i` -, none when pool_of[b] == -1."""
import numpy as np
import pandas as pd

SLABS = 512


def n_options(g, with_doublets):
    return g * (g + 1) // 2 if with_doublets else g


def enumerate_options(g, with_doublets):
    """[(i,) or (i, j)] per pool-local option."""
    options = [(i,) for i in range(g)]
    if with_doublets:
        options += [(i, j) for i in range(g) for j in range(i + 1, g)]
    return options


def row_pointer(pool_sizes, pool_of, with_doublets):
    widths = [n_options(pool_sizes[p], with_doublets) if p >= 0 else 0 for p in pool_of]
    return np.concatenate([[0], np.cumsum(widths)]).astype(np.int64)


def rows_of(pool_of, pool):
    return np.flatnonzero(np.asarray(pool_of) == pool)


def pool_frame(values, row_ptr, pool_of, pool):
    """[n_p, K_p]: the rows of the pool's barcodes in ascending barcode order."""
    rows = rows_of(pool_of, pool)
    if len(rows) == 0:
        return np.zeros((0, 0), dtype=values.dtype)
    return np.stack([values[row_ptr[b]:row_ptr[b + 1]] for b in rows])


def first_maximum(values, offset=0):
    """(index + offset, value) of the first maximum; a NaN never wins; (-1, NaN) when nothing is left."""
    best, best_value = -1, np.float32(np.nan)
    for k, v in enumerate(values):
        if v != v:
            continue
        if best < 0 or v > best_value:
            best, best_value = k + offset, v
    return best, best_value


def sequential(values):
    total = np.float64(0)
    for v in values:
        total = total + np.float64(v)
    return total


def readout(probs, row_ptr, pool_of, pool_sizes, with_doublets):
    """dict of what dmx_pooled_readout returns, marg_ptr and the compact donor_marginals among it."""
    probs = np.asarray(probs)
    assert probs.dtype == np.float32
    B = len(pool_of)
    out = dict(singlet_mass=np.full(B, np.nan), doublet_mass=np.full(B, np.nan))
    for name in ('best_option', 'best_singlet', 'best_pair'):
        out[name] = np.full(B, -1, dtype=np.int32)
    for name in ('best_prob', 'best_singlet_prob', 'best_pair_prob'):
        out[name] = np.full(B, np.nan, dtype=np.float32)
    marg_ptr, marginals = [0], []
    for b in range(B):
        p = pool_of[b]
        if p < 0:
            marg_ptr.append(marg_ptr[-1])
            continue
        g = pool_sizes[p]
        row = probs[row_ptr[b]:row_ptr[b + 1]]
        options = enumerate_options(g, with_doublets)
        assert len(row) == len(options)
        out['singlet_mass'][b] = sequential(row[:g])
        out['doublet_mass'][b] = sequential(row[g:])
        out['best_option'][b], out['best_prob'][b] = first_maximum(row)
        out['best_singlet'][b], out['best_singlet_prob'][b] = first_maximum(row[:g])
        out['best_pair'][b], out['best_pair_prob'][b] = first_maximum(row[g:], g)
        if len(row) == g:
            out['best_pair'][b] = -1
        if with_doublets:
            containing = [[] for _ in range(g)]
            for k, option in enumerate(options):  # ascending option order
                for donor in option:
                    containing[donor].append(k)
            marginals.extend(np.float32(sequential(row[k] for k in containing[i])) for i in range(g))
        else:
            marginals.extend(row)
        marg_ptr.append(marg_ptr[-1] + g)
    out['marg_ptr'] = np.asarray(marg_ptr, dtype=np.int64)
    out['donor_marginals'] = np.asarray(marginals, dtype=np.float32)
    return out


def top_options(probs, row_ptr, k):
    """(int32[B, k], float32[B, k]): best first, ties to the lower index, NaNs never; -1 / NaN where the row runs out."""
    B = len(row_ptr) - 1
    options, values = np.full((B, k), -1, dtype=np.int32), np.full((B, k), np.nan, dtype=np.float32)
    for b in range(B):
        row = probs[row_ptr[b]:row_ptr[b + 1]]
        ranked = sorted((i for i in range(len(row)) if row[i] == row[i]), key=lambda i: (-np.float64(row[i]), i))
        for j, i in enumerate(ranked[:k]):
            options[b, j], values[b, j] = i, row[i]
    return options, values


def slab_sum(values):
    """The float64 sum of a list in the fixed order of dmx_get_option_sums: 512 slabs of ceil(n / 512) positions each added
    sequentially, then the slab sums in slab order."""
    n = len(values)
    per = -(-n // SLABS)
    total = np.float64(0)
    for j in range(SLABS):
        total = total + sequential(values[min(j * per, n):min((j + 1) * per, n)])
    return total


def option_sums(probs, row_ptr, pool_of, pool_sizes, with_doublets):
    """(float64 sums pool after pool, int64[P] barcodes per pool)."""
    sums, counts = [], []
    for p, g in enumerate(pool_sizes):
        frame = pool_frame(probs, row_ptr, pool_of, p)
        counts.append(len(frame))
        K = n_options(g, with_doublets)
        sums.extend(slab_sum(frame[:, k]) if len(frame) else np.float64(0) for k in range(K))
    return np.asarray(sums, dtype=np.float64), np.asarray(counts, dtype=np.int64)


def allowed_mass(probs, row_ptr, pool_of, start, options):
    """(mass float64[B], best_is_allowed int32[B]); NaN / 0 for a barcode in no pool."""
    B = len(pool_of)
    mass, hit = np.full(B, np.nan), np.zeros(B, dtype=np.int32)
    for b in range(B):
        if pool_of[b] < 0:
            continue
        row = probs[row_ptr[b]:row_ptr[b + 1]]
        listed = [int(k) for k in options[start[b]:start[b + 1]]]
        mass[b] = sequential(row[k] for k in listed)
        hit[b] = first_maximum(row)[0] in listed
    return mass, hit


def calls(r, pool_of, pool_names, pool_donors, with_doublets, threshold):
    """DevicePooledPosteriors.droplet_calls from a restated readout r: per barcode, with its own pool's donor names."""
    rows = []
    for b, p in enumerate(pool_of):
        if p < 0:
            rows.append((None, 'unassigned', None, None, np.nan, np.nan))
            continue
        donors = pool_donors[p]
        options = enumerate_options(len(donors), with_doublets)
        s, sp, mass = r['best_singlet'][b], r['best_singlet_prob'][b], r['doublet_mass'][b]
        if s >= 0 and sp > np.float32(threshold):
            rows.append((pool_names[p], 'singlet', donors[s], None, np.float64(sp), mass))
        elif r['best_pair'][b] >= 0 and mass > threshold:
            i, j = options[r['best_pair'][b]]
            rows.append((pool_names[p], 'doublet', donors[i], donors[j], mass, mass))
        else:
            rows.append((pool_names[p], 'unassigned', None, None, np.fmax(np.float64(sp), mass), mass))
    return pd.DataFrame(rows, columns=['pool', 'status', 'donor_1', 'donor_2', 'probability', 'doublet_probability'])


def summary(frame, sums, pool_names, pool_donors, with_doublets):
    """DevicePooledPosteriors.donor_summary from calls()' frame and option_sums()' sums: indexed by (pool, donor)."""
    records, first = [], 0
    for name, donors in zip(pool_names, pool_donors):
        options = enumerate_options(len(donors), with_doublets)
        mine = frame[frame['pool'] == name]
        for i, donor in enumerate(donors):
            expected = np.float64(0)
            for k, option in enumerate(options):
                if i in option:
                    expected = expected + sums[first + k]
            records.append((name, donor, int(((mine['status'] == 'singlet') & (mine['donor_1'] == donor)).sum()),
                            int(((mine['status'] == 'doublet') & ((mine['donor_1'] == donor) | (mine['donor_2'] == donor))).sum()), expected))
        first += len(options)
    out = pd.DataFrame(records, columns=['pool', 'donor', 'n_singlets', 'n_doublets', 'expected_cells'])
    return out.set_index(['pool', 'donor'])
