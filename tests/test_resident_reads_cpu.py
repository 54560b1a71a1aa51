"""Resident read sets without a GPU: every new C entry point refuses its arguments before it touches a device, ResidentReads
and the fronts that take it check types and state up to the point where a device is needed, and the host restatement of the
largest reference_end (what dmx_reads_info reports) is the one both CIGAR walkers agree on."""
import ctypes

import numpy as np
import pytest

from demuxalot_amd import DecodedReads, ReadCounter, ResidentReads, _lib, count_snps_from_reads, coverage_from_reads, find_candidate_positions
from demuxalot_amd.snp_detection import reference_ends
from tests import coverage_restatement as cr
from tests.test_coverage_cpu import RestatementContext

NEW_ENTRY_POINTS = ('dmx_reads_upload', 'dmx_reads_release', 'dmx_reads_info', 'dmx_count_reads_resident', 'dmx_coverage_count_resident',
                    'dmx_count_reads_push_resident', 'dmx_get_reads_upload_bytes')


def test_new_entry_points_are_declared_bound_and_documented():
    """(tests/test_host_cpu.py checks declared == bound == exported for both headers; this adds where and how they are declared.)"""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'demux_hip_debug.h')).read()
    public = open(os.path.join(root, 'include', 'demux_hip.h')).read()
    lib = _lib.load()
    for name in NEW_ENTRY_POINTS:
        assert name in _lib.DEBUG_SIGNATURES and name not in _lib.SIGNATURES
        assert f'int {name}(' in header and f'int {name}(' not in public
        assert list(getattr(lib, name).argtypes) == list(_lib.DEBUG_SIGNATURES[name][1])
    # the binding passes the context first, handles and sizes as int64, and one int64 per name of READS_INFO
    assert _lib.READS_INFO == ('n_reads', 'n_cigar_ops', 'n_bases', 'nbytes', 'reference_length')
    assert _lib.DEBUG_SIGNATURES['dmx_reads_info'][1][1:] == [ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]


def test_c_entry_points_validate_their_arguments_without_a_gpu():
    lib = _lib.load()
    n, handle = ctypes.c_int64(0), ctypes.c_int64(7)
    info = (ctypes.c_int64 * 5)()
    table = np.ones(41)
    desc = _lib.DecodedReadsStruct(n_reads=0, n_cigar_ops=0, n_bases=0)
    reads = ctypes.cast(ctypes.byref(desc), ctypes.c_void_p)
    # a null context, with every other argument valid
    assert lib.dmx_reads_upload(None, reads, ctypes.byref(handle)) != 0
    assert lib.dmx_reads_release(None, 1) != 0
    assert lib.dmx_reads_info(None, 1, info) != 0
    assert lib.dmx_count_reads_resident(None, 1, None, 0, _lib.ptr(table), ctypes.byref(n), ctypes.byref(n)) != 0
    assert lib.dmx_coverage_count_resident(None, 1, 0, 10, 15, None) != 0
    assert lib.dmx_count_reads_push_resident(None, 1, 0, 0, 0, ctypes.byref(n), ctypes.byref(n)) != 0
    assert lib.dmx_get_reads_upload_bytes(None, ctypes.byref(n)) != 0
    # ... and null pointers, negative ranges and windows on top of it: refused, nothing is dereferenced
    assert lib.dmx_reads_upload(None, None, None) != 0
    assert lib.dmx_reads_info(None, -1, None) != 0
    assert lib.dmx_count_reads_resident(None, -1, None, -1, None, None, None) != 0
    assert lib.dmx_coverage_count_resident(None, -1, -1, -2, 256, None) != 0
    assert lib.dmx_count_reads_push_resident(None, -1, -5, -9, 0, None, None) != 0
    assert lib.dmx_get_reads_upload_bytes(None, None) != 0
    assert b'null ctx' in lib.dmx_last_error()


def reads():
    return DecodedReads(**cr.make_reads([(5, '2S 3M 4D 2M 10N 1M 2H', 'AAAAAAAA', 30), (7, '1M', 'A', 30), (9, '3= 2X 1I', 'AAAAAA', 30)]))


def unopened():
    """A ResidentReads as close() leaves it (none can be uploaded without a device)."""
    resident = ResidentReads.__new__(ResidentReads)
    resident._ctx = resident._handle = None
    resident._shared, resident._coverage_only = True, False
    return resident


def test_resident_reads_type_and_state_errors():
    for wrong in (reads().arrays(), None, 5):
        with pytest.raises(TypeError, match='DecodedReads'):
            ResidentReads(wrong)
    if _lib.device_count() == 0:
        with pytest.raises(_lib.DemuxHipError, match='no HIP device'):  # the upload needs a device: no quiet stand-in
            ResidentReads(reads())
    closed = unopened()
    assert closed.closed
    closed.close()  # idempotent, and it needs no device
    for use in (lambda: closed.n_reads, lambda: closed.nbytes, lambda: closed.reference_length, closed.__enter__,
                lambda: count_snps_from_reads({'c': closed}, {'c': np.array([1], np.int32)}),
                lambda: count_snps_from_reads({'c': closed}, {'c': np.array([1], np.int32)}, on_context=object()),
                lambda: coverage_from_reads(closed, 0, 4), lambda: find_candidate_positions({'c': closed}, minimum_coverage=1)):
        with pytest.raises(ValueError, match='closed'):
            use()


def test_a_set_runs_on_its_own_context_only():
    mine, other = object(), object()
    resident = unopened()
    resident._ctx, resident._handle, resident._shared = mine, 3, False
    resident._info = dict(n_reads=2, n_cigar_ops=2, n_bases=8, nbytes=100, reference_length=12)
    try:
        assert (resident.n_reads, resident.nbytes, resident.reference_length) == (2, 100, 12)
        for use in (lambda: count_snps_from_reads({'c': resident}, {'c': np.array([1], np.int32)}, on_context=other),
                    lambda: coverage_from_reads(resident, 0, 4, on_context=other),
                    lambda: find_candidate_positions({'c': resident}, minimum_coverage=1, on_context=other)):
            with pytest.raises(ValueError, match='another context'):
                use()
        elsewhere = unopened()
        elsewhere._ctx, elsewhere._handle, elsewhere._shared, elsewhere._info = other, 4, False, dict(resident._info)
        with pytest.raises(ValueError, match='one context'):
            find_candidate_positions({'a': resident, 'b': elsewhere}, minimum_coverage=1)
        elsewhere._handle = None
        with pytest.raises(ValueError, match='beyond 2\\^31'):
            resident._info['reference_length'] = 2 ** 31
            find_candidate_positions({'c': resident}, minimum_coverage=1, on_context=mine)
    finally:
        resident._handle = None  # (nothing to release)


def test_read_counter_takes_ranges_of_resident_reads_only():
    counter = ReadCounter(np.array([1], np.int32), on_context=object())
    counter._ctx = object()  # as inside its with block
    for wrong in ((reads(), 0, 1), (unopened(),), 'chr1'):
        with pytest.raises(TypeError):
            counter.push(wrong)
    with pytest.raises(ValueError, match='closed'):
        counter.push((unopened(), 0, 1))
    with pytest.raises(ValueError, match='closed'):
        counter.finish(unopened())


def test_host_reads_keep_their_path_on_a_context_that_holds_no_reads():
    """find_candidate_positions on a stand-in context (coverage_count of host arrays only) counts as before, and refuses a
    cigar range outside the array before anything is counted."""
    ctx = RestatementContext()
    got = find_candidate_positions({'chr1': reads()}, minimum_coverage=0, minimum_alternative_coverage=0, max_fragment_step=7, on_context=ctx)
    assert ctx.windows == [(0, 7), (7, 14), (14, 21), (21, 25)] and int(reference_ends(reads()).max()) == 25
    assert got['chr1'].dtype == np.int32
    broken = reads()
    broken.n_cigar[2] = 9
    ctx = RestatementContext()
    with pytest.raises(ValueError, match='cigar range'):
        find_candidate_positions({'chr1': broken}, minimum_coverage=1, on_context=ctx)
    assert ctx.windows == []
