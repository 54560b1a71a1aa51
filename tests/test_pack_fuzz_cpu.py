"""The pack problems of tests/pack_problems.py on the CPU: the host twin of the device pack (dmx_pack_calls_host,
csrc/pack_host.cpp) against the oracle on every case, and the cases themselves - every edge the table is there for must
be in it.  What tests/test_gpu_pack_fuzz.py then runs on the GPU is known to be a problem on which the generator and the
oracle agree."""
import collections
import ctypes

import numpy as np
import pytest

from tests import fixture_io as fio
from tests import pack_problems as pp


def host_pack(prob):
    from demuxalot_amd import _lib
    n, V = prob.n_calls, prob.n_variants
    call_variant = np.empty(n, dtype=np.int32)
    out_v, out_cb = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    out_p, out_count = np.empty(n, dtype=np.float32), np.empty(n, dtype=np.int64)
    mol = np.zeros(V, dtype=np.int64)
    n_matched, n_unique = ctypes.c_int64(0), ctypes.c_int64(0)
    ptr = _lib.ptr
    _lib.check(_lib.load().dmx_pack_calls_host(
        V, ptr(prob.var_chrom), ptr(prob.var_pos), ptr(prob.var_base), n, ptr(prob.chrom), ptr(prob.pos), ptr(prob.base), ptr(prob.cb),
        ptr(prob.p), ptr(call_variant), ctypes.byref(n_matched), ctypes.byref(n_unique), ptr(out_v), ptr(out_cb), ptr(out_p),
        ptr(out_count), ptr(mol)))
    k = n_unique.value
    return call_variant, n_matched.value, k, out_v[:k], out_cb[:k], out_p[:k], out_count[:k], mol


@pytest.mark.parametrize('name', list(pp.CASES))
def test_host_pack_matches_oracle(oracle, name):
    prob, want = pp.problem(name), pp.expected_of(name, oracle)
    call_variant, n_matched, n_unique, variant, cb, p, count, mol = host_pack(prob)
    assert np.array_equal(call_variant, want.call_variant)
    assert (n_matched, n_unique) == (want.n_matched, want.n_unique)
    assert np.array_equal(variant, want.variant) and np.array_equal(cb, want.cb) and np.array_equal(count, want.count)
    fio.assert_bitwise(p, want.p, f'{name}: p_base_wrong products')
    assert np.array_equal(mol, want.mol_per_variant)


@pytest.mark.parametrize('name', list(pp.CASES))
def test_containers_hold_the_flat_calls(name):
    """The two forms of a problem are the same calls in the same order; chromosomes, barcodes and sizes are in range."""
    prob = pp.problem(name)
    case = pp.CASES[name]
    assert (prob.n_variants, prob.n_calls, prob.n_barcodes) == (case['V'], case['n_calls'], case['n_barcodes'])
    for flat, packed in zip((prob.chrom, prob.pos, prob.base, prob.cb, prob.p), pp.flat_from_containers(prob)):
        assert flat.dtype == packed.dtype and np.array_equal(flat, packed)
    assert prob.n_calls == 0 or (prob.cb.min() >= 0 and prob.cb.max() < prob.n_barcodes)
    assert len(prob.v2snp) == prob.n_variants and prob.n_calls <= 300000 and prob.n_variants <= 70000


def test_negative_barcodes_as_the_host_twin_treats_them(oracle):
    """What the GPU test's refusals rest on (pack_host.cpp): a negative barcode on a matched call is refused, on an
    unmatched call it is dropped with the call."""
    from demuxalot_amd import _lib
    prob, want = pp.problem('n512'), pp.expected_of('n512', oracle)
    matched, unmatched = int(np.flatnonzero(want.call_variant >= 0)[3]), int(np.flatnonzero(want.call_variant < 0)[3])
    with pytest.raises(_lib.DemuxHipError, match=r'negative barcode.*status -1\)'):
        host_pack(pp.with_barcode(prob, matched, -1))
    other = pp.with_barcode(prob, unmatched, -1)
    for flat, packed in zip((other.chrom, other.pos, other.base, other.cb, other.p), pp.flat_from_containers(other)):
        assert np.array_equal(flat, packed)
    got = host_pack(other)
    assert got[1:3] == (want.n_matched, want.n_unique) and np.array_equal(got[3], want.variant) and np.array_equal(got[4], want.cb)
    fio.assert_bitwise(got[5], want.p, 'a negative barcode on an unmatched call')


def test_cases_exercise_the_contract(oracle):
    """Every named case of the table is hit, with the counts it is there for (computed from the inputs and the
    oracle's output, never from the library)."""
    hits = {name: pp.cases_hit(pp.problem(name), pp.expected_of(name, oracle), oracle) for name in pp.CASES}
    total, most = collections.Counter(), collections.Counter()
    for name, hit in hits.items():
        print(name, dict(hit))
        total.update(hit)
        for case, count in hit.items():
            most[case] = max(most[case], count)
    print('in one case at most:', dict(most))
    # sizes at block and bit edges
    for n in (0, 1, 255, 256, 257, 511, 512, 513):
        assert total[f'n_calls={n}'], n
    for m in ('0 of some', '1', '256', '257'):
        assert total[f'matched={m}'], m
    for V in (1, 2, 31, 32, 33, 1023, 1024, 1025, 32767, 32768, 65537):
        assert total[f'V={V}'], V
    assert total['table of 64 slots'] >= 3 and total['table half full'] >= 3   # V = 1, 2, 31 (2 V = 64 takes 128 slots); V = 2^k - 1
    for B in (1, 2, 256, 257, 4097):
        assert total[f'n_barcodes={B}'], B
    big = [name for name, hit in hits.items() if hit['n_barcodes=4097'] or hit['n_barcodes=257'] or hit['n_barcodes=256']]
    assert all(hits[name]['calls on the last barcode'] for name in big if hits[name].get('matched=0 of some', 0) == 0 and pp.CASES[name]['n_calls'] > 1)
    assert sum(1 for name in big if hits[name]['barcodes without calls']) >= 5
    # runs of equal (variant, barcode)
    for length in pp.RUN_LENGTHS:
        assert most[f'run of {length}'] >= 20, length
    assert total['run of 5000'] == 2
    assert most['product depends on the order'] >= 1000 and most['run scattered through the call order'] >= 1000
    assert total['run from the last 10 slots of a block into the next'] >= 20
    assert total['first run has several members'] >= 8 and total['last run has several members'] >= 8
    assert total['every call in one run'] == 1 and total['every call unique'] == 1
    # float32 products
    assert most['subnormal product'] >= 20 and most['product underflows to 0'] >= 6
    assert min(most['member 0'], most['member 1'], most['member 1e-38']) >= 2
    # matching
    assert total['site with the bases 0..4'] >= len(pp.CASES) - 3   # (every case with 6 variants at least)
    for case in ('call at a variant position with another base', 'call on a listed chromosome at a position without variants'):
        assert most[case] >= 1000 and sum(1 for hit in hits.values() if hit[case]) >= 10, case
    assert total['matched call at position 0'] >= 20 and total['matched call at position 2^31 - 1'] >= 20
    assert total['var_chrom not sorted'] >= 12 and total['three chromosomes'] >= 12 and total['about 30 % unmatched'] >= 6
    wrapping = [name for name, hit in hits.items() if hit['variant in the last table slot'] >= 3]
    assert len(wrapping) >= 10
    for name in wrapping:
        if hits[name].get('about 30 % unmatched'):
            assert hits[name]['matched call on a variant of the last table slot'] >= 3 and hits[name]['unmatched call in the last table slot'] >= 3, name
    # containers
    for name, hit in hits.items():
        assert hit['container with 0 calls'] >= 1 and hit['empty container on a chromosome without variants'] == 1, name
        if pp.CASES[name]['n_calls'] >= 255:
            assert hit['chromosome split over two containers'] == 1 and hit['container order differs from the numbering'] == 1, name
            assert hit['molecule table larger than the calls use'] >= 2 and hit['molecule with several calls'] >= 10, name
