"""Learning within pools (include/demux_hip_debug.h: dmx_em_pools; Demultiplexer.learn_genotypes_in_pools) restated with the
oracle, used as the checker by tests/test_pools_learning_cpu.py and tests/test_gpu_pools_learning.py.

The reference's loop (demux.py:86-118) with its E-step replaced by the pooled one.  Per iteration:
    prob     = oracle.probs_from_betas(v2snp, betas + addition, clip)
    rows     = pools_restatement.Restatement on that table: every barcode's row is the row of its pool
    dense    = float32[B, G]: dense[b, d_p[i]] = row_b[i] for i < g_p, everything else +0 (a barcode of pool -1 included)
    addition = oracle.beta_addition(v, cb, e, dense, V, G, power)
Adding (0 * keep) ** power = +0 to a float64 sum changes nothing, so the zero-filled matrix is the same as leaving those calls out.
With one all-donor pool this is the reference's staged_genotype_learning itself (tests/test_pools_learning_cpu.py).  Nothing here knows
the library."""
import numpy as np

from oracle import demux_oracle
from tests import fixture_io as fio
from tests import pools_restatement as restated


def fixture_learning_problem(name):
    """dict(v, cb, e, v2snp, betas, raw_betas, B) of a golden fixture as learn_genotypes sees it (prior betas with the data term)."""
    fx = fio.load(name)
    return dict(v=fx['pack_bc_variant_id'], cb=fx['pack_bc_cb'], e=fx['pack_bc_p'], v2snp=fx['pack_v2snp'], betas=fx['pack1_betas'],
                raw_betas=fx['betas'], B=len(fx['barcodes']))


def dense_singlets(rows, pools, pool_of_barcode, B, G):
    """The [B, G] matrix the M-step reads, from the compact rows of one pooled E-step."""
    pool_of_barcode = np.asarray(pool_of_barcode, dtype=np.int32)
    dense = np.zeros((B, G), dtype=np.float32)
    for p, donors in enumerate(pools):
        members = np.flatnonzero(pool_of_barcode == p)
        if not len(members):
            continue
        take = rows['row_ptr'][members][:, None] + np.arange(len(donors), dtype=np.int64)[None, :]
        dense[members[:, None], np.asarray(donors, dtype=np.int64)[None, :]] = rows['probs'][take]
    return dense


def learn(problem, pools, pool_of_barcode, n_iterations, clip, doublet_prior, power=2.):
    """Per iteration a dict: the pooled E-step's row_ptr / logits / probs / best_option / best_prob / doublet_mass, `dense`, the `addition` its
    E-step used and the genotype table `prob_table`."""
    v, cb, e, v2snp, betas, B = (problem[k] for k in ('v', 'cb', 'e', 'v2snp', 'betas', 'B'))
    V, G = betas.shape
    addition = np.zeros_like(betas)
    history = []
    for _it in range(n_iterations):
        prob = demux_oracle.probs_from_betas(v2snp, betas + addition, clip)
        rows = restated.Restatement(v, cb, e, prob, B, doublet_prior)(pools, pool_of_barcode)
        dense = dense_singlets(rows, pools, pool_of_barcode, B, G)
        history.append(dict(rows, dense=dense, addition=addition, prob_table=prob))
        addition = demux_oracle.beta_addition(v, cb, e, dense, V, G, power=power)
    return history


def learnt_betas(problem, history):
    """genotypes.get_betas() + the addition the last E-step used (demux.py:65)."""
    return problem['raw_betas'] + history[-1]['addition']
