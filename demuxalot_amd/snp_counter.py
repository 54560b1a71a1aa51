"""CompressedSNPCalls: the input wire format of the hot path (mirror of the container at
demuxalot/snp_counter.py:77-139), and the step that fills it: the compute half of the reference's count_snps
(snp_counter.py:37-69, 142-276) on the GPU, from reads the caller has decoded (include/demux_hip.h "Read counting",
csrc/count_reads.hip; the contract is in DESIGN.md "Read counting").  Reading and decompressing BAM files stays with the caller.

Two structured arrays whose first n_* entries are valid:
  molecules  (compressed_cb i32, compressed_ub i32, p_group_misaligned f32)
  snp_calls  (molecule_index i32, snp_position i32, base_index u8, p_base_wrong f32)
Demultiplexer reads only `[:n]` slices, so objects produced by the reference's count_snps can
be passed in unchanged (duck typing).  from_arrays builds a container from plain columns, concatenate joins the
containers of the regions of one chromosome, count_snps_from_reads produces them from DecodedReads."""
import numpy as np

from .device import get_context, shared_context_lock

MOLECULE_DTYPE = np.dtype([('compressed_cb', 'int32'), ('compressed_ub', 'int32'), ('p_group_misaligned', 'float32')])
SNP_CALL_DTYPE = np.dtype([('molecule_index', 'int32'), ('snp_position', 'int32'), ('base_index', 'uint8'),
                           ('p_base_wrong', 'float32')])


class CompressedSNPCalls:
    def __init__(self, start_snps_size=1024, start_molecule_size=128):
        self.n_molecules = 0
        self.molecules = np.zeros(start_molecule_size, dtype=MOLECULE_DTYPE)
        self.molecules[:] = (-1, -1, -1.)
        self.n_snp_calls = 0
        self.snp_calls = np.zeros(start_snps_size, dtype=SNP_CALL_DTYPE)
        self.snp_calls[:] = (-1, -1, 255, -1.)

    @staticmethod
    def from_arrays(compressed_cb, snp_calls_molecule_index, snp_position, base_index, p_base_wrong,
                    compressed_ub=None, p_group_misaligned=0.01) -> 'CompressedSNPCalls':
        """Builds a container from plain arrays (used by tests, fixtures and the synthetic generator)."""
        out = CompressedSNPCalls(start_snps_size=1, start_molecule_size=1)
        out.molecules = np.zeros(len(compressed_cb), dtype=MOLECULE_DTYPE)
        out.molecules['compressed_cb'] = compressed_cb
        out.molecules['compressed_ub'] = np.arange(len(compressed_cb)) if compressed_ub is None else compressed_ub
        out.molecules['p_group_misaligned'] = p_group_misaligned
        out.snp_calls = np.zeros(len(snp_position), dtype=SNP_CALL_DTYPE)
        out.snp_calls['molecule_index'] = snp_calls_molecule_index
        out.snp_calls['snp_position'] = snp_position
        out.snp_calls['base_index'] = base_index
        out.snp_calls['p_base_wrong'] = p_base_wrong
        out.n_molecules, out.n_snp_calls = len(out.molecules), len(out.snp_calls)
        return out

    def minimize_memory_footprint(self):
        """Drops the unused tail of both arrays (snp_counter.py:114-118)."""
        self.snp_calls = self.snp_calls[:self.n_snp_calls].copy()
        self.molecules = self.molecules[:self.n_molecules].copy()
        assert np.all(self.molecules['p_group_misaligned'] != -1)
        assert np.all(self.snp_calls['p_base_wrong'] != -1)

    @staticmethod
    def concatenate(snp_calls_list) -> 'CompressedSNPCalls':
        """Joins containers of the same chromosome, in the list's order (snp_counter.py:120-139): the molecule indices of
        every part are shifted by the molecules before it."""
        molecules, snp_calls, n_molecules = [], [], 0
        for part in snp_calls_list:
            calls = part.snp_calls[:part.n_snp_calls].copy()
            calls['molecule_index'] += n_molecules
            snp_calls.append(calls)
            molecules.append(part.molecules[:part.n_molecules])
            n_molecules += part.n_molecules
        out = CompressedSNPCalls(start_snps_size=1, start_molecule_size=1)
        out.molecules = np.concatenate(molecules)
        out.snp_calls = np.concatenate(snp_calls)
        out.n_molecules, out.n_snp_calls = len(out.molecules), len(out.snp_calls)
        return out


QUALITY_CAP = 40  # base qualities count up to this (snp_counter.py:172)


def quality_table():
    """float64[41]: probability that a base of quality q is wrong, with the reference's expression (snp_counter.py:172)."""
    return np.array([0.1 ** (0.1 * q) for q in range(QUALITY_CAP + 1)], dtype=np.float64)


class DecodedReads:
    """The reads of one chromosome that the reference's scanner would keep (parse_read(read) and
    barcode_handler.get_barcode_index(read) both not None), in fetch order, as plain arrays that mirror a BAM record:

      per read  reference_start i32, compressed_cb i32, compressed_ub i32, p_misaligned f64, alignment_score i32 (AS),
                cigar_begin i64, n_cigar i32, seq_begin i64, l_seq i32
      cigar     u32, BAM-encoded (length << 4 | op); read r owns cigar[cigar_begin[r] : cigar_begin[r] + n_cigar[r]]
      seq       u8, ASCII letters; qual u8; read r owns [seq_begin[r] : seq_begin[r] + l_seq[r]] of both
    """
    PER_READ = (('reference_start', np.int32), ('compressed_cb', np.int32), ('compressed_ub', np.int32),
                ('p_misaligned', np.float64), ('alignment_score', np.int32), ('cigar_begin', np.int64), ('n_cigar', np.int32),
                ('seq_begin', np.int64), ('l_seq', np.int32))
    FLAT = (('cigar', np.uint32), ('seq', np.uint8), ('qual', np.uint8))

    def __init__(self, **arrays):
        expected = [name for name, _ in self.PER_READ + self.FLAT]
        if sorted(arrays) != sorted(expected):
            raise TypeError(f'DecodedReads takes exactly the arrays {expected}')
        for name, dtype in self.PER_READ + self.FLAT:
            value = np.ascontiguousarray(arrays[name], dtype=dtype)
            if value.ndim != 1:
                raise ValueError(f'{name} must be one-dimensional')
            setattr(self, name, value)
        for name, _ in self.PER_READ:
            if len(getattr(self, name)) != len(self.reference_start):
                raise ValueError(f'{name} has {len(getattr(self, name))} entries for {len(self.reference_start)} reads')
        if len(self.seq) != len(self.qual):
            raise ValueError('seq and qual must have the same length')
        if self.n_reads >= 2 ** 31:
            raise ValueError('at most 2^31 - 1 reads per call')

    @property
    def n_reads(self):
        return len(self.reference_start)

    def arrays(self):
        return {name: getattr(self, name) for name, _ in self.PER_READ + self.FLAT}

    def slice(self, lo, hi) -> 'DecodedReads':
        """The reads [lo, hi) (as a Python slice clips them) with cigar_begin and seq_begin re-based to arrays of their own: a
        chunk of a stream (ReadCounter).  On the host; the reads' cigar and seq ranges must be non-decreasing in read order, as
        from_reads and a BAM decoder lay them out."""
        lo, hi, _ = slice(lo, hi).indices(self.n_reads)
        hi = max(lo, hi)
        columns = {name: getattr(self, name)[lo:hi] for name, _ in self.PER_READ}
        if hi == lo:
            return DecodedReads(cigar=self.cigar[:0], seq=self.seq[:0], qual=self.qual[:0], **columns)
        c0, s0 = int(self.cigar_begin[lo]), int(self.seq_begin[lo])
        c1, s1 = int(self.cigar_begin[hi - 1]) + int(self.n_cigar[hi - 1]), int(self.seq_begin[hi - 1]) + int(self.l_seq[hi - 1])
        if np.any(np.diff(columns['cigar_begin']) < 0) or np.any(np.diff(columns['seq_begin']) < 0):
            raise ValueError('slice needs cigar_begin and seq_begin non-decreasing in read order')
        columns['cigar_begin'] = columns['cigar_begin'] - c0
        columns['seq_begin'] = columns['seq_begin'] - s0
        return DecodedReads(cigar=self.cigar[c0:c1], seq=self.seq[s0:s1], qual=self.qual[s0:s1], **columns)

    @staticmethod
    def from_reads(reads, barcode_handler, parse_read) -> 'DecodedReads':
        """From an iterable of pysam-like reads (reference_start, cigartuples, seq, query_qualities, get_tag, has_tag, mapq),
        with the two filters of the reference's scanner (snp_counter.py:251-256).  Host Python: for tests and for callers who
        read their BAM files with pysam."""
        columns = {name: [] for name, _ in DecodedReads.PER_READ}
        cigar, seq, qual = [], [], []
        n_cigar_total = n_seq_total = 0
        for read in reads:
            parsed = parse_read(read)
            if parsed is None:
                continue
            cb = barcode_handler.get_barcode_index(read)
            if cb is None:
                continue
            p_misaligned, ub = parsed
            ops = [(int(length) << 4) | int(op) for op, length in read.cigartuples]
            letters = np.frombuffer(read.seq.encode('ascii'), dtype=np.uint8)
            qualities = np.asarray(read.query_qualities, dtype=np.uint8)
            if len(qualities) != len(letters):
                raise ValueError('a read has a different number of bases and qualities')
            for name, value in (('reference_start', read.reference_start), ('compressed_cb', cb), ('compressed_ub', ub),
                                ('p_misaligned', p_misaligned), ('alignment_score', read.get_tag('AS')),
                                ('cigar_begin', n_cigar_total), ('n_cigar', len(ops)), ('seq_begin', n_seq_total),
                                ('l_seq', len(letters))):
                columns[name].append(value)
            cigar.append(np.asarray(ops, dtype=np.uint32))
            seq.append(letters)
            qual.append(qualities)
            n_cigar_total += len(ops)
            n_seq_total += len(letters)

        def flat(parts, dtype):
            return np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype=dtype)
        return DecodedReads(cigar=flat(cigar, np.uint32), seq=flat(seq, np.uint8), qual=flat(qual, np.uint8), **columns)


class ResidentReads:
    """The arrays of one chromosome's DecodedReads uploaded ONCE to a device context and accepted wherever a DecodedReads is:
    counting, coverage, candidate search and detection then move no read to the device (include/demux_hip_debug.h
    "Resident reads"; DESIGN.md "Resident reads").  A context manager:

        with ResidentReads(decoded) as resident:
            calls = count_snps_from_reads({'chr1': resident}, {'chr1': positions})
            candidates = find_candidate_positions({'chr1': resident}, minimum_coverage=200)

    Without on_context the set lives on the shared context, and every call that takes it runs there under the shared lock;
    with one, on that context (the caller holds it) - a call that names another context raises ValueError.  The set keeps
    no reference to the host arrays.  coverage_only leaves compressed_cb, compressed_ub, p_misaligned and alignment_score
    on the host: such a set serves coverage_from_reads and find_candidate_positions, counting on it fails."""

    def __init__(self, reads, on_context=None, *, coverage_only=False):
        self._ctx = self._handle = None
        if not isinstance(reads, DecodedReads):
            raise TypeError('reads must be a DecodedReads')
        self._shared = on_context is None
        self._coverage_only = bool(coverage_only)

        def upload(ctx):
            handle = ctx.reads_upload(reads, coverage_only=self._coverage_only)
            return ctx, handle, ctx.reads_info(handle)

        if self._shared:
            with shared_context_lock:
                self._ctx, self._handle, self._info = upload(get_context())
        else:
            self._ctx, self._handle, self._info = upload(on_context)

    def _check(self, on_context=None):
        if self._handle is None:
            raise ValueError('this ResidentReads is closed')
        if on_context is not None and on_context is not self._ctx:
            raise ValueError('this ResidentReads lives on another context than the one the call runs on')

    @property
    def closed(self):
        """True once close() has run (or the with block was left); every other use then raises ValueError."""
        return self._handle is None

    @property
    def coverage_only(self):
        """True for a set uploaded without the four counting columns."""
        return self._coverage_only

    @property
    def n_reads(self):
        self._check()
        return self._info['n_reads']

    @property
    def nbytes(self):
        """Device bytes the set holds."""
        self._check()
        return self._info['nbytes']

    @property
    def reference_length(self):
        """The largest reference_end of the reads (0 without reads), found on the device when the set was uploaded."""
        self._check()
        return max(0, self._info['reference_length'])

    def close(self):
        ctx, handle, self._handle = self._ctx, self._handle, None
        if handle is None or getattr(ctx, '_h', None) is None:  # (a destroyed context has freed its sets)
            return
        if self._shared:
            with shared_context_lock:
                ctx.reads_release(handle)
        else:
            ctx.reads_release(handle)

    def __enter__(self):
        self._check()
        return self

    def __exit__(self, *_exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class ResidentCalls:
    """The two record arrays of one chromosome's CompressedSNPCalls held on a device context and accepted wherever the container
    is: Demultiplexer.predict_posteriors / learn_genotypes / staged_genotype_learning, select_snps_from_calls,
    detect_snps_positions_from_calls, calls_per_barcode, summarize_counted_SNPs - none of which then moves a call record over the
    link (include/demux_hip_debug.h "Resident calls"; DESIGN.md "Resident calls").  ResidentCalls(container) uploads a host
    container; count_snps_from_reads(..., resident_calls=True) and ReadCounter(keep_calls=True) leave the counted records in such
    sets without a download.  A set is immutable; a context manager:

        with ResidentCalls(container) as resident:
            logits, probs = Demultiplexer.predict_posteriors({'chr1': resident}, genotypes, handler)

    Without on_context the set lives on the shared context.  Consumers may run on another context of the same device.  There is no
    .snp_calls / .molecules: to_host() is the (explicit) download.  Every use after close() raises RuntimeError."""

    def __init__(self, container, on_context=None):
        self._ctx = self._handle = None
        if isinstance(container, ResidentCalls):
            raise TypeError('container is a ResidentCalls already (concatenate([it]) makes a copy on the device)')
        try:
            n_calls, n_molecules = int(container.n_snp_calls), int(container.n_molecules)
            snp_calls, molecules = container.snp_calls, container.molecules
        except AttributeError:
            raise TypeError('container must be a CompressedSNPCalls (snp_calls, n_snp_calls, molecules, n_molecules)') from None
        if getattr(snp_calls, 'dtype', None) != SNP_CALL_DTYPE or getattr(molecules, 'dtype', None) != MOLECULE_DTYPE:
            raise TypeError("the container's record arrays must have the dtypes SNP_CALL_DTYPE and MOLECULE_DTYPE")
        if not (0 <= n_calls <= len(snp_calls) and 0 <= n_molecules <= len(molecules)):
            raise ValueError('n_snp_calls / n_molecules do not fit the record arrays')
        if on_context is None:
            with shared_context_lock:
                ctx = get_context()
                self._adopt_handle(ctx, ctx.calls_upload(snp_calls[:n_calls], molecules[:n_molecules]))
        else:
            self._adopt_handle(on_context, on_context.calls_upload(snp_calls[:n_calls], molecules[:n_molecules]))

    def _adopt_handle(self, ctx, handle):
        """Takes over a SEALED set of ctx (the caller holds ctx)."""
        self._shared = bool(getattr(ctx, '_is_shared', False))
        try:
            self._info, self._device_view = ctx.calls_info(handle), ctx.calls_view(handle)
        except BaseException:
            ctx.calls_release(handle)
            raise
        self._ctx, self._handle = ctx, handle

    @classmethod
    def _adopt(cls, ctx, handle):
        out = cls.__new__(cls)
        out._ctx = out._handle = None
        out._adopt_handle(ctx, handle)
        return out

    def __getattr__(self, name):  # (only reached for names that are not there)
        if name in ('snp_calls', 'molecules'):
            raise AttributeError(f'a ResidentCalls keeps its records on the device and has no .{name}: to_host() downloads them')
        raise AttributeError(f'{type(self).__name__!r} object has no attribute {name!r}')

    def _check(self):
        if self._handle is None:
            raise RuntimeError('this ResidentCalls is closed')
        if getattr(self._ctx, '_h', None) is None:
            raise RuntimeError('the device context of this ResidentCalls was destroyed, and the set with it')

    def _locked(self, run):
        self._check()
        if self._shared:
            with shared_context_lock:
                return run(self._ctx)
        return run(self._ctx)

    def _view(self, on_device=None):
        """The set's device pointers and sizes, for a consumer on `on_device` (another device: TypeError)."""
        self._check()
        if on_device is not None and int(on_device) != self._ctx.device:
            raise TypeError(f'this ResidentCalls lives on device {self._ctx.device}, the call runs on device {int(on_device)}')
        return self._device_view

    @property
    def closed(self):
        """True once close() has run (or the with block was left)."""
        return self._handle is None

    @property
    def n_molecules(self):
        self._check()
        return self._info['n_molecules']

    @property
    def n_snp_calls(self):
        self._check()
        return self._info['n_snp_calls']

    @property
    def nbytes(self):
        """Device bytes the set holds."""
        self._check()
        return self._info['nbytes']

    def to_host(self) -> 'CompressedSNPCalls':
        """The records as a CompressedSNPCalls: the one download of a set."""
        return _container(*self._locked(lambda ctx: ctx.calls_fetch(self._handle)))

    def barcode_counts(self, n_barcodes):
        """(calls int64[n_barcodes], molecules int64[n_barcodes]) per compressed_cb, counted on the device."""
        return self._locked(lambda ctx: ctx.calls_barcode_counts(self._handle, n_barcodes))

    @staticmethod
    def concatenate(resident_calls_list) -> 'ResidentCalls':
        """CompressedSNPCalls.concatenate on the device: a new set on the parts' context, the parts in list order."""
        parts = list(resident_calls_list)
        if not parts or not all(isinstance(part, ResidentCalls) for part in parts):
            raise TypeError('concatenate takes a non-empty list of ResidentCalls')
        for part in parts:
            part._check()
            if part._ctx is not parts[0]._ctx:
                raise ValueError('the ResidentCalls of one concatenate must live on one context')
        if sum(part.n_molecules for part in parts) >= 2 ** 31:
            raise ValueError('2^31 molecules or more: molecule_index is an int32')
        return parts[0]._locked(lambda ctx: ResidentCalls._adopt(ctx, ctx.calls_concatenate([part._handle for part in parts])))

    def close(self):
        ctx, handle, self._handle = self._ctx, self._handle, None
        if handle is None or getattr(ctx, '_h', None) is None:  # (a destroyed context has freed its sets)
            return
        if self._shared:
            with shared_context_lock:
                ctx.calls_release(handle)
        else:
            ctx.calls_release(handle)

    def __enter__(self):
        self._check()
        return self

    def __exit__(self, *_exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def split_call_sets(chromosome2calls, what='chromosome2compressed_snp_calls'):
    """True when every value of the dict is a ResidentCalls, False when none is; a dict that mixes the two kinds is a TypeError."""
    kinds = {isinstance(calls, ResidentCalls) for calls in chromosome2calls.values()}
    if len(kinds) == 2:
        raise TypeError(f'{what} mixes ResidentCalls and host containers: pass one kind (to_host() / ResidentCalls(container) convert)')
    return kinds == {True}


def _container(molecules, snp_calls):
    out = CompressedSNPCalls(start_snps_size=1, start_molecule_size=1)
    out.molecules, out.snp_calls = molecules, snp_calls
    out.n_molecules, out.n_snp_calls = len(molecules), len(snp_calls)
    return out


def _empty_container():
    return _container(np.zeros(0, dtype=MOLECULE_DTYPE), np.zeros(0, dtype=SNP_CALL_DTYPE))


class ReadCounter:
    """The reads of ONE chromosome counted in chunks, in device memory bounded by the chunk and the molecules still open
    (include/demux_hip_debug.h "Streamed read counting"; DESIGN.md "Read counting", "Streaming").  A context manager:

        with ReadCounter(positions) as counter:
            for chunk in chunks:                      # DecodedReads, in read order
                molecules, snp_calls = counter.push(chunk)
            molecules, snp_calls = counter.finish()

    push returns the records of the molecules that chunk's reads flushed, finish the rest; concatenated they are the records of
    count_snps_from_reads on all the reads (molecule_index counts on across the pushes).  Without on_context the shared context
    is used and its lock is held from __enter__ to __exit__.  One stream per context.
    keep_calls=True: the records stay on the device - push and finish return (n_molecules, n_snp_calls) of that push, and after
    finish() `.calls` is the sealed ResidentCalls of the whole stream (the caller's: it outlives the with block)."""

    def __init__(self, positions, on_context=None, keep_calls=False):
        self._positions = np.ascontiguousarray(positions, dtype=np.int32)
        self._on_context = on_context
        self._ctx = None
        self._finished = False
        self._keep_calls = bool(keep_calls)
        self._set = None   # handle of the open set the pushes fill (keep_calls)
        self.calls = None  # keep_calls: the sealed ResidentCalls, once finish() has run

    def __enter__(self):
        if self._ctx is not None:
            raise RuntimeError('this ReadCounter is open already')
        locked = self._on_context is None
        if locked:
            shared_context_lock.acquire()
        try:
            ctx = get_context() if locked else self._on_context
            ctx.count_reads_begin(self._positions, quality_table())
            if self._keep_calls:
                try:
                    self._set = ctx.calls_open()
                except BaseException:
                    ctx.count_reads_end()
                    raise
        except BaseException:
            if locked:
                shared_context_lock.release()
            raise
        self._ctx, self._finished = ctx, False
        self.calls = None
        return self

    def __exit__(self, *_exc):
        ctx, self._ctx = self._ctx, None
        handle, self._set = self._set, None
        try:
            try:
                if handle is not None:  # left before finish(): the half-filled set goes
                    ctx.calls_release(handle)
            finally:
                ctx.count_reads_end()
        finally:
            if self._on_context is None:
                shared_context_lock.release()

    def _push(self, reads, final):
        if self._ctx is None:
            raise RuntimeError('ReadCounter is a context manager: push inside its with block')
        if self._finished:
            raise RuntimeError('this ReadCounter has finished')
        if isinstance(reads, ResidentReads):
            reads = (reads, 0, reads.n_reads)
        if isinstance(reads, tuple):
            if len(reads) != 3 or not isinstance(reads[0], ResidentReads):
                raise TypeError('a device range is (ResidentReads, first_read, last_read)')
            resident, lo, hi = reads
            resident._check(self._ctx)
            out = self._ctx.count_reads_push_resident(resident._handle, lo, hi, final=final, fetch=not self._keep_calls)
        elif reads is not None and not isinstance(reads, DecodedReads):
            raise TypeError('a chunk must be a DecodedReads, a ResidentReads or a (ResidentReads, first_read, last_read) range')
        else:
            out = self._ctx.count_reads_push(reads, final=final, fetch=not self._keep_calls)
        if self._keep_calls:
            self._ctx.calls_append_counted(self._set)
            if final:
                self._ctx.calls_seal(self._set)
                handle, self._set = self._set, None
                self.calls = ResidentCalls._adopt(self._ctx, handle)
        self._finished = final
        return out

    def push(self, reads):
        """(molecules, snp_calls) of the molecules the reads of this chunk flushed.  reads: a DecodedReads, or reads that are
        on the counter's context already: a ResidentReads (all of it) or a (ResidentReads, first_read, last_read) range."""
        return self._push(reads, False)

    def finish(self, reads=None):
        """(molecules, snp_calls) of a last chunk (optional) and of every molecule still open."""
        return self._push(reads, True)

    @property
    def carried_reads(self):
        """Reads the last push left on the device: those of the molecules still open."""
        return 0 if self._ctx is None else self._ctx.count_reads_carry()


def _count_chunks(ctx, chunks, positions, resident_calls=False):
    """One chromosome's container (resident_calls: ResidentCalls) from an iterable of chunks, one chunk alive at a time."""
    molecules, snp_calls = [], []
    with ReadCounter(positions, on_context=ctx, keep_calls=resident_calls) as counter:
        iterator = iter(chunks)
        while True:
            chunk = next(iterator, None)
            part = counter.finish() if chunk is None else counter.push(chunk)
            molecules.append(part[0])
            snp_calls.append(part[1])
            if chunk is None:
                break
            del chunk
    if resident_calls:
        return counter.calls
    return _container(np.concatenate(molecules), np.concatenate(snp_calls))


def _empty_resident(ctx):
    handle = ctx.calls_open()
    ctx.calls_seal(handle)
    return ResidentCalls._adopt(ctx, handle)


def _counted_resident(ctx, count):
    """The records count(fetch=False) leaves on ctx, as a sealed ResidentCalls."""
    count(fetch=False)
    handle = ctx.calls_open()
    try:
        ctx.calls_append_counted(handle)
        ctx.calls_seal(handle)
    except BaseException:
        ctx.calls_release(handle)
        raise
    return ResidentCalls._adopt(ctx, handle)


def _closing_on_failure(run):
    """run(ctx) -> dict of results; the ResidentCalls it had made are closed when it raises."""
    def guarded(ctx):
        result = {}
        try:
            run(ctx, result)
        except BaseException:
            for calls in result.values():
                if isinstance(calls, ResidentCalls):
                    calls.close()
            raise
        return result
    return guarded


def _on(on_context, run, reads=()):
    """run(ctx) on the context the call belongs to: on_context (the caller holds it), else the context of the ResidentReads
    among `reads` (the shared one under its lock), else the shared context under its lock."""
    sets = [r for r in reads if isinstance(r, ResidentReads)]
    for resident in sets:
        resident._check(on_context)
        if resident._ctx is not sets[0]._ctx:
            raise ValueError('the ResidentReads of one call must live on one context')
    if on_context is not None:
        return run(on_context)
    if sets and not sets[0]._shared:
        return run(sets[0]._ctx)
    with shared_context_lock:
        ctx = get_context()
        if sets and sets[0]._ctx is not ctx:
            raise ValueError('the shared context these ResidentReads were uploaded to is no longer the shared context')
        return run(ctx)


def count_snps_from_read_chunks(chromosome2chunks, chromosome2positions, *, on_context=None, resident_calls=False):
    """count_snps_from_reads for reads that arrive in batches: chromosome2chunks maps a chromosome to an iterable of
    DecodedReads (a generator is fine), the chunks of that chromosome in read order.  Every iterable is consumed lazily, one
    chunk alive at a time, so neither the host nor the device ever holds a whole chromosome (ReadCounter).

    :param resident_calls: as for count_snps_from_reads
    :return: what count_snps_from_reads returns on the concatenated chunks.  A chromosome without chunks gives an empty
        container; the chunks of a chromosome without positions are consumed and skipped.
    """
    if not isinstance(chromosome2chunks, dict) or not isinstance(chromosome2positions, dict):
        raise TypeError('chromosome2chunks and chromosome2positions must be dicts keyed by chromosome')

    def run(ctx, result):
        for chromosome, positions in chromosome2positions.items():
            chunks = chromosome2chunks.get(chromosome)
            if chunks is None:
                result[chromosome] = _empty_resident(ctx) if resident_calls else _empty_container()
            else:
                result[chromosome] = _count_chunks(ctx, chunks, positions, resident_calls)
        for chromosome, chunks in chromosome2chunks.items():
            if chromosome not in chromosome2positions:
                for _chunk in chunks:
                    pass

    return _on(on_context, _closing_on_failure(run))


def count_snps_from_reads(chromosome2reads, chromosome2positions, *, on_context=None, max_reads_per_call=None, resident_calls=False):
    """count_snps (snp_counter.py:279-327) with the BAM reading replaced by reads the caller has decoded: per chromosome of
    chromosome2positions (in its order) one device call that groups the reads into molecules, walks the CIGARs to the
    SNP positions, multiplies the base-error probabilities and resolves conflicting bases (DESIGN.md "Read counting").

    :param chromosome2reads: dict chromosome -> DecodedReads (reference_start non-decreasing) or ResidentReads (the reads are
        on the device already: nothing is uploaded, and the call runs on their context)
    :param chromosome2positions: dict chromosome -> strictly ascending zero-based SNP positions
    :param on_context: a DeviceContext to run on (the caller holds it); default: the shared context, under its lock
    :param max_reads_per_call: None: one device call per chromosome.  A number: every chromosome is cut into slices of at most
        that many reads and streamed (ReadCounter), which bounds the device memory by the slice; the result is the same.  The
        slices of a ResidentReads are ranges on the device, cut where the host slices are.
    :param resident_calls: True: the values of the result are ResidentCalls on the counting context - the records stay on the
        device, nothing is fetched; they are the caller's to close()
    :return: dict chromosome -> CompressedSNPCalls, record for record what the reference's count_call_variants_for_chromosome
        returns.  A chromosome without reads gives an empty container; reads of a chromosome without positions are skipped.
    """
    if not isinstance(chromosome2reads, dict) or not isinstance(chromosome2positions, dict):
        raise TypeError('chromosome2reads and chromosome2positions must be dicts keyed by chromosome')
    if max_reads_per_call is not None and int(max_reads_per_call) < 1:
        raise ValueError('max_reads_per_call must be at least 1')
    table = quality_table()

    def run(ctx, result):
        for chromosome, positions in chromosome2positions.items():
            reads = chromosome2reads.get(chromosome)
            if reads is not None and not isinstance(reads, (DecodedReads, ResidentReads)):
                raise TypeError(f'chromosome2reads[{chromosome!r}] must be a DecodedReads or a ResidentReads')
            resident = isinstance(reads, ResidentReads)
            if reads is None or reads.n_reads == 0:
                result[chromosome] = _empty_resident(ctx) if resident_calls else _empty_container()
            elif max_reads_per_call is None:
                def count(fetch=True, reads=reads, positions=positions):
                    if resident:
                        return ctx.count_reads_resident(reads._handle, positions, table, fetch=fetch)
                    return ctx.count_reads(reads, positions, table, fetch=fetch)
                result[chromosome] = _counted_resident(ctx, count) if resident_calls else _container(*count())
            else:
                step, n = int(max_reads_per_call), reads.n_reads
                if resident:
                    chunks = ((reads, lo, min(lo + step, n)) for lo in range(0, n, step))
                else:
                    chunks = (reads.slice(lo, lo + step) for lo in range(0, n, step))
                result[chromosome] = _count_chunks(ctx, chunks, positions, resident_calls)

    return _on(on_context, _closing_on_failure(run), [chromosome2reads.get(chromosome) for chromosome in chromosome2positions])
