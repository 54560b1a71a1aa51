"""Plain Python restatement of the STREAMED read-counting contract (DESIGN.md "Read counting", "Streaming"): test code the
device's stream and the golden fixtures are compared with.  A push works on carry + chunk: carried reads are never events, the
chunk's first read is an event iff it is the first read of the stream or enters another 1000-base segment than the last read
of the previous non-empty chunk; a molecule that no event of the push flushes is not emitted, its reads become the next carry.

What an emitted molecule holds (duplicates, p_group_misaligned, observations, folds, the order of its calls) is not restated
here: every emitted molecule's reads go through count_reads of tests/count_reads_restatement.py, which gives exactly one
group for reads of one (cb, ub) key with no other read between them (a split needs an event BETWEEN two reads of the key)."""
import numpy as np

from demuxalot_amd.snp_counter import MOLECULE_DTYPE, SNP_CALL_DTYPE, DecodedReads
from tests.count_reads_restatement import SEGMENT, InvalidReads, count_reads, reference_end

PER_READ = [name for name, _ in DecodedReads.PER_READ]
EMPTY = DecodedReads(**{name: np.zeros(0, dtype) for name, dtype in DecodedReads.PER_READ + DecodedReads.FLAT}).arrays()


def take(reads, members):
    """The reads `members` (ascending indices) of a dict of arrays, as a dict of arrays of its own (begins re-based)."""
    members = np.asarray(members, dtype=np.int64)
    out = {name: np.asarray(reads[name])[members] for name in PER_READ}
    for begin, count, flats in (('cigar_begin', 'n_cigar', ('cigar',)), ('seq_begin', 'l_seq', ('seq', 'qual'))):
        pieces = [(int(reads[begin][r]), int(reads[begin][r]) + int(reads[count][r])) for r in members]
        for flat in flats:
            parts = [np.asarray(reads[flat])[lo:hi] for lo, hi in pieces]
            out[flat] = np.concatenate(parts) if parts else np.asarray(reads[flat])[:0]
        lengths = np.array([hi - lo for lo, hi in pieces], dtype=np.int64)
        out[begin] = (np.cumsum(lengths) - lengths).astype(np.int64)
    return out


def joined(a, b):
    """carry + chunk: the reads of b behind those of a."""
    out = {name: np.concatenate([a[name], b[name]]) for name in PER_READ + ['cigar', 'seq', 'qual']}
    out['cigar_begin'] = np.concatenate([a['cigar_begin'], np.asarray(b['cigar_begin'], dtype=np.int64) + len(a['cigar'])])
    out['seq_begin'] = np.concatenate([a['seq_begin'], np.asarray(b['seq_begin'], dtype=np.int64) + len(a['seq'])])
    return out


def chunk_of(reads, lo, hi):
    return take(reads, np.arange(lo, hi))


class StreamRestatement:
    def __init__(self, positions, table=None):
        self.positions, self.table = np.asarray(positions), table
        self.carry = EMPTY
        self.previous_start = None  # reference_start of the last read of the last non-empty chunk: the one carried integer
        self.n_molecules = 0
        self.finished = False
        self.largest_carry = 0

    @property
    def carried_reads(self):
        return len(self.carry['reference_start'])

    def push(self, chunk=None, final=False):
        """(molecules, snp_calls) this push emits; molecule_index counts on across pushes."""
        if self.finished:
            raise InvalidReads('push after the final push')
        chunk = EMPTY if chunk is None else chunk
        start_of_chunk = np.asarray(chunk['reference_start'], dtype=np.int64)
        if np.any(start_of_chunk[1:] < start_of_chunk[:-1]):
            raise InvalidReads('reference_start decreases')
        if len(start_of_chunk) and self.previous_start is not None and start_of_chunk[0] < self.previous_start:
            raise InvalidReads('the chunk starts below the previous chunk\'s last read')
        n_carry = self.carried_reads
        reads = joined(self.carry, chunk)
        start = np.asarray(reads['reference_start'], dtype=np.int64)
        n = len(start)

        def is_event(r):
            if r < n_carry:
                return False
            before = self.previous_start if r == n_carry else start[r - 1]
            return before is None or start[r] // SEGMENT != before // SEGMENT

        open_groups = {}  # key -> [members, reach], in the order the molecules were opened: by first read
        emitted = []
        for r in range(n):
            key = (int(reads['compressed_cb'][r]), int(reads['compressed_ub'][r]))
            group = open_groups.setdefault(key, [[], -2 ** 63])
            group[0].append(r)
            group[1] = max(group[1], reference_end(reads, r))
            if is_event(r):  # (after the read has joined its molecule: a read never flushes the molecule it belongs to)
                threshold = int(start[r]) - SEGMENT
                for key in [key for key, (_members, reach) in open_groups.items() if reach < threshold]:
                    emitted.append(open_groups.pop(key)[0])
        # (a dict keeps insertion order and a molecule is inserted at its first read: every flush above, and the final one
        # below, lists its molecules by first read - carried molecules first, in their original order)
        if final:
            emitted.extend(members for members, _reach in open_groups.values())
            open_groups = {}
            self.finished = True
        molecules, snp_calls = [], []
        for members in emitted:
            one, calls = count_reads(take(reads, members), self.positions, self.table)
            assert len(one) <= 1
            if len(one):
                calls = calls.copy()
                calls['molecule_index'] = self.n_molecules
                self.n_molecules += 1
                molecules.append(one)
                snp_calls.append(calls)
        self.carry = take(reads, sorted(r for members, _reach in open_groups.values() for r in members))
        self.largest_carry = max(self.largest_carry, self.carried_reads)
        if len(start_of_chunk):
            self.previous_start = int(start_of_chunk[-1])
        return (np.concatenate(molecules) if molecules else np.zeros(0, MOLECULE_DTYPE),
                np.concatenate(snp_calls) if snp_calls else np.zeros(0, SNP_CALL_DTYPE))


def count_reads_streamed(reads, positions, cuts, table=None, carries=None):
    """(molecules, snp_calls) of the reads pushed as the chunks [0, cuts[0]), [cuts[0], cuts[1]), ..., [cuts[-1], n); the last
    chunk is the final push.  carries: a list that receives the carry after every push."""
    n = len(reads['reference_start'])
    bounds = [0] + [int(c) for c in cuts] + [n]
    stream = StreamRestatement(positions, table)
    parts = []
    for k, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
        parts.append(stream.push(chunk_of(reads, lo, hi), final=k == len(bounds) - 2))
        if carries is not None:
            carries.append(stream.carried_reads)
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def even_cuts(n, n_chunks):
    return [n * k // n_chunks for k in range(1, n_chunks)]
