"""Resident call sets, what needs no device (include/demux_hip_debug.h "Resident calls"; demuxalot_amd/snp_counter.py:
ResidentCalls): where the entry points are declared, the argument and type errors that are decided before a context is
touched, the host side of calls_per_barcode / summarize_counted_SNPs against np.bincount and collections.Counter, and that the
resident key of a problem packed from ResidentCalls is built without looking at a record."""
import collections
import os
import re

import numpy as np
import pytest

from demuxalot_amd import CompressedSNPCalls, Demultiplexer, ResidentCalls, calls_per_barcode, summarize_counted_SNPs
from demuxalot_amd.snp_counter import MOLECULE_DTYPE, SNP_CALL_DTYPE, _container, split_call_sets
from tests import fixture_io as fio
from tests.test_count_reads_cpu import FIXTURES, fixture_chromosomes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('dmx_calls_upload', 'dmx_calls_open', 'dmx_calls_append_counted', 'dmx_calls_seal', 'dmx_calls_concatenate',
                'dmx_calls_view', 'dmx_calls_info', 'dmx_calls_fetch', 'dmx_calls_release', 'dmx_calls_barcode_counts',
                'dmx_stage_device_containers', 'dmx_snp_count_device', 'dmx_get_calls_transfer_bytes')


def closed_set(handle=None):
    """A ResidentCalls no device ever saw: closed, or - with a handle - just the name of a set."""
    out = ResidentCalls.__new__(ResidentCalls)
    out._ctx = None
    out._handle = handle
    return out


def test_the_debug_header_declares_the_block_and_the_public_header_none_of_it():
    from demuxalot_amd import _lib
    debug = open(os.path.join(ROOT, 'include', 'demux_hip_debug.h')).read()
    public = open(os.path.join(ROOT, 'include', 'demux_hip.h')).read()
    assert re.search(r'^ \* Resident calls \(product API', debug, flags=re.M)
    for name in ENTRY_POINTS:
        assert re.search(rf'^int {name}\(', debug, flags=re.M), name
        assert name in _lib.DEBUG_SIGNATURES and name not in _lib.SIGNATURES
        assert name not in public
    block = debug[debug.index(' * Resident calls (product API'):]
    for word in ('sealed', 'never\n * reused', 'dmx_release_problem leaves them', 'hipPointerGetAttributes', 'DMX_ERR_UNSUPPORTED'):
        assert word in block, word


def test_argument_and_type_errors_are_raised_before_a_device_is_touched():
    good = CompressedSNPCalls.from_arrays([0], [0], [5], [1], [0.01])
    with pytest.raises(TypeError, match='CompressedSNPCalls'):
        ResidentCalls(object())
    with pytest.raises(TypeError, match='ResidentCalls already'):
        ResidentCalls(closed_set())
    wrong = CompressedSNPCalls.from_arrays([0], [0], [5], [1], [0.01])
    wrong.snp_calls = wrong.snp_calls.astype([('molecule_index', 'int64'), ('snp_position', 'int32'), ('base_index', 'uint8'),
                                              ('p_base_wrong', 'float32')])
    with pytest.raises(TypeError, match='SNP_CALL_DTYPE'):
        ResidentCalls(wrong)
    too_many = CompressedSNPCalls.from_arrays([0], [0], [5], [1], [0.01])
    too_many.n_snp_calls = 2
    with pytest.raises(ValueError, match='do not fit'):
        ResidentCalls(too_many)
    for bad in ([], [good], [closed_set(), good]):
        with pytest.raises(TypeError, match='non-empty list of ResidentCalls'):
            ResidentCalls.concatenate(bad)
    # a closed set: every use raises RuntimeError, the record arrays do not exist and the error says where they are
    closed = closed_set()
    assert closed.closed
    for use in (lambda: closed.n_molecules, lambda: closed.n_snp_calls, lambda: closed.nbytes, closed.to_host,
                lambda: closed.barcode_counts(3), closed.__enter__, lambda: ResidentCalls.concatenate([closed]),
                lambda: summarize_counted_SNPs({'chr1': closed}), lambda: calls_per_barcode({'chr1': closed}, 3)):
        with pytest.raises(RuntimeError, match='closed'):
            use()
    closed.close()  # (closing twice is fine)
    for name in ('snp_calls', 'molecules'):
        with pytest.raises(AttributeError, match=r'to_host\(\)'):
            getattr(closed, name)
    assert not hasattr(closed, 'snp_calls') and not hasattr(closed, 'no_such_thing')
    # a set of another device than the consumer's
    import types
    elsewhere = closed_set(handle=3)
    elsewhere._ctx, elsewhere._device_view = types.SimpleNamespace(device=1, _h=1), 'the view'
    assert elsewhere._view(1) == 'the view' and elsewhere._view() == 'the view'
    with pytest.raises(TypeError, match='lives on device 1, the call runs on device 0'):
        elsewhere._view(0)
    elsewhere._handle = None
    # one kind per dict
    assert split_call_sets({'a': closed, 'b': closed_set()}) is True and split_call_sets({'a': good}) is False
    assert split_call_sets({}) is False
    for consumer in (lambda mixed: Demultiplexer.pack_calls(mixed, None, True), lambda mixed: calls_per_barcode(mixed, 4),
                     split_call_sets):
        with pytest.raises(TypeError, match='mixes ResidentCalls and host containers'):
            consumer({'chr1': good, 'chr2': closed})
    # the multi-GPU entry points say that they are out of scope
    from demuxalot_amd import distributed
    with pytest.raises(TypeError, match='out of scope for the multi-GPU entry points'):
        distributed._install_shard({'chr1': closed}, None, None, None, True, None, 'f64', None, False)


def host_containers(name):
    if name.startswith('f9'):
        return {chromosome: _container(molecules, snp_calls) for chromosome, _reads, _positions, molecules, snp_calls in fixture_chromosomes(name)}
    return fio.product_inputs(fio.load(name))[0]


@pytest.mark.parametrize('name', FIXTURES + ('f6_shipped_example.npz',))
def test_the_summaries_of_host_containers_equal_bincount_and_counter(name):
    counts = host_containers(name)
    n_barcodes = 1 + max(int(c.molecules['compressed_cb'][:c.n_molecules].max()) for c in counts.values())
    calls, transcripts = calls_per_barcode(counts, n_barcodes)
    assert calls.dtype == np.int64 and transcripts.dtype == np.int64 and calls.shape == transcripts.shape == (n_barcodes,)
    # the reference's two Counters (utils.py:168-180) ...
    barcode2calls, barcode2transcripts = collections.Counter(), collections.Counter()
    want_calls, want_transcripts = np.zeros(n_barcodes, np.int64), np.zeros(n_barcodes, np.int64)
    for c in counts.values():
        molecules, snp_calls = c.molecules[:c.n_molecules], c.snp_calls[:c.n_snp_calls]
        barcode2transcripts.update(collections.Counter(molecules['compressed_cb'].tolist()))
        barcode2calls.update(collections.Counter(molecules['compressed_cb'][snp_calls['molecule_index']].tolist()))
        # ... and np.bincount
        want_transcripts += np.bincount(molecules['compressed_cb'], minlength=n_barcodes)
        want_calls += np.bincount(molecules['compressed_cb'][snp_calls['molecule_index']], minlength=n_barcodes)
    assert np.array_equal(calls, want_calls) and np.array_equal(transcripts, want_transcripts)
    assert {b: int(n) for b, n in enumerate(calls) if n} == dict(barcode2calls)
    assert {b: int(n) for b, n in enumerate(transcripts) if n} == dict(barcode2transcripts)
    assert calls.sum() == sum(c.n_snp_calls for c in counts.values()) > 0
    with pytest.raises(ValueError, match='compressed_cb outside'):
        calls_per_barcode(counts, n_barcodes - 1)
    frame = summarize_counted_SNPs(counts)
    assert list(frame.index) == sorted(counts) and frame.index.name == 'chromosome'
    assert list(frame.columns) == ['n_molecules', 'n_snp_calls']
    for chromosome, c in counts.items():
        assert tuple(frame.loc[chromosome]) == (c.n_molecules, c.n_snp_calls)
    # containers with a spare tail, as count_snps leaves them before minimize_memory_footprint: only [:n] counts
    padded = {}
    for chromosome, c in counts.items():
        padded[chromosome] = CompressedSNPCalls(start_snps_size=c.n_snp_calls + 7, start_molecule_size=c.n_molecules + 3)
        padded[chromosome].snp_calls[:c.n_snp_calls], padded[chromosome].molecules[:c.n_molecules] = c.snp_calls[:c.n_snp_calls], c.molecules[:c.n_molecules]
        padded[chromosome].n_snp_calls, padded[chromosome].n_molecules = c.n_snp_calls, c.n_molecules
    again = calls_per_barcode(padded, n_barcodes)
    assert np.array_equal(again[0], calls) and np.array_equal(again[1], transcripts)


def test_the_resident_key_is_built_without_touching_a_record():
    """Handles are never reused and sealed sets never change: the key names the sets, it hashes nothing."""
    from demuxalot_amd.demux import _resident_calls_key, _var2varid_fingerprint

    class Untouchable:
        """Stands where a ResidentCalls stands; its records raise when anything looks at them."""

        def __init__(self, handle):
            self._handle = handle

        def __getattr__(self, name):
            raise AssertionError(f'the key looked at .{name}')

    _calls, genotypes, handler = fio.product_inputs(fio.load('f3_small_0.npz'))
    named = [('chr2', Untouchable(41)), ('chr1', Untouchable(7))]
    key = _resident_calls_key(named, genotypes, handler.n_barcodes, False)
    assert key == ('resident-calls', (('chr2', 41), ('chr1', 7)), _var2varid_fingerprint(genotypes.var2varid), genotypes.n_variants,
                   genotypes.n_genotypes, handler.n_barcodes, False)
    assert key == _resident_calls_key(list(named), genotypes, handler.n_barcodes, False)
    # everything the key is made of changes it: a handle, the order, the chromosome, the shape, the mapping, the switch
    others = [_resident_calls_key([('chr2', Untouchable(41)), ('chr1', Untouchable(8))], genotypes, handler.n_barcodes, False),
              _resident_calls_key(named[::-1], genotypes, handler.n_barcodes, False),
              _resident_calls_key([('chr3', named[0][1]), named[1]], genotypes, handler.n_barcodes, False),
              _resident_calls_key(named, genotypes, handler.n_barcodes + 1, False),
              _resident_calls_key(named, genotypes, handler.n_barcodes, True)]
    changed = genotypes.clone()
    changed.var2varid = dict(genotypes.var2varid)
    others.append(_resident_calls_key(named, changed, handler.n_barcodes, False))
    assert all(other != key for other in others) and len(set(others)) == len(others)
    # the same holds for the real type: a ResidentCalls has no record arrays to look at
    real = [('chr1', closed_set(handle=5))]
    assert _resident_calls_key(real, genotypes, handler.n_barcodes, False)[1] == (('chr1', 5),)
    assert MOLECULE_DTYPE.itemsize == 12 and SNP_CALL_DTYPE.itemsize == 13
