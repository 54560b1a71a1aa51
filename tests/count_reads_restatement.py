"""Plain Python / numpy restatement of the read-counting contract (DESIGN.md "Read counting"): test code that the device
path and the golden fixtures are compared with, written from the contract's definitions (events, groups, duplicates,
observations, per-position folds, order keys) and not as a scan with a dictionary of open groups."""
import bisect

import numpy as np

from demuxalot_amd.snp_counter import MOLECULE_DTYPE, SNP_CALL_DTYPE, quality_table

SEGMENT = 1000
BOTH, REFERENCE_ONLY, READ_ONLY = (0, 7, 8), (2, 3), (1, 4, 5, 6)
BASE_CODE = {ord(letter): code for code, letter in enumerate('ACGTN')}


class InvalidReads(ValueError):
    """What the C entry point answers with its invalid-argument status."""


def _ops(reads, r):
    begin, n = int(reads['cigar_begin'][r]), int(reads['n_cigar'][r])
    return [(int(c) & 0xF, int(c) >> 4) for c in reads['cigar'][begin:begin + n]]


def reference_end(reads, r):
    return int(reads['reference_start'][r]) + sum(length for op, length in _ops(reads, r) if op in BOTH + REFERENCE_ONLY)


def observations(reads, r, positions):
    """[(position, letter, quality)] of read r, position ascending."""
    out = []
    ref_cursor, read_cursor = int(reads['reference_start'][r]), 0
    seq_begin, l_seq = int(reads['seq_begin'][r]), int(reads['l_seq'][r])
    for op, length in _ops(reads, r):
        if op in BOTH:
            lo, hi = np.searchsorted(positions, [ref_cursor, ref_cursor + length], side='left')
            for position in positions[lo:hi]:
                i = read_cursor + int(position) - ref_cursor
                if not 0 <= i < l_seq:
                    raise InvalidReads(f'read {r}: base {i} of {l_seq} at position {position}')
                letter = int(reads['seq'][seq_begin + i])
                if letter not in BASE_CODE:
                    raise InvalidReads(f'read {r}: letter {chr(letter)!r} at position {position}')
                out.append((int(position), letter, int(reads['qual'][seq_begin + i])))
            ref_cursor += length
            read_cursor += length
        elif op in REFERENCE_ONLY:
            ref_cursor += length
        elif op in READ_ONLY:
            read_cursor += length
        else:
            raise InvalidReads(f'read {r}: CIGAR operation {op}')
    return out


def count_reads(reads, positions, table=None, trace=None):
    """(molecules, snp_calls) structured arrays of the contract; `reads` maps the names of DecodedReads to arrays.
    trace: a collections.Counter that receives how often every special case of the contract occurred."""
    trace = {} if trace is None else trace

    def saw(what):
        trace[what] = trace.get(what, 0) + 1
    table = quality_table() if table is None else table
    positions = np.asarray(positions, dtype=np.int64)
    start = np.asarray(reads['reference_start'], dtype=np.int64)
    n = len(start)
    if np.any(start[1:] < start[:-1]):
        raise InvalidReads('reference_start decreases')
    end = [reference_end(reads, r) for r in range(n)]
    events = [e for e in range(n) if e == 0 or start[e] // SEGMENT != start[e - 1] // SEGMENT]
    threshold = [int(start[e]) - SEGMENT for e in events]  # non-decreasing

    by_key = {}
    for r in range(n):
        by_key.setdefault((int(reads['compressed_cb'][r]), int(reads['compressed_ub'][r])), []).append(r)

    def flushing_event(last_read, reach):
        """Number (in `events`) of the first event after last_read whose threshold is above reach; len(events): none."""
        first_after = bisect.bisect_right(events, last_read)
        return max(first_after, bisect.bisect_right(threshold, reach))

    groups = []  # (flushing event, first read, key, members)
    for key, members in by_key.items():
        current, reach = [members[0]], end[members[0]]
        for b in members[1:]:
            between = bisect.bisect_left(events, b) - 1  # the last event before b
            if between >= 0 and events[between] > current[-1] and reach < threshold[between]:
                groups.append((flushing_event(current[-1], reach), current[0], key, current))
                current, reach = [b], end[b]
                saw('key split into molecules')
            else:
                if between >= 0 and events[between] > current[-1]:
                    saw('event inside a molecule')
                current.append(b)
                reach = max(reach, end[b])
        groups.append((flushing_event(current[-1], reach), current[0], key, current))
    groups.sort(key=lambda g: g[:2])

    molecules, snp_calls = [], []
    for _event, _first, (cb, ub), members in groups:
        seen, p_group = set(), 1.0
        per_position = {}  # position -> (rank of the first read that saw it, {letter: product}); dicts keep insertion order
        rank = 0
        for r in members:
            identity = (int(start[r]), end[r], int(reads['alignment_score'][r]))
            if identity in seen:
                saw('complete duplicate')
                continue
            if any(other[:2] == identity[:2] for other in seen):
                saw('same span, other alignment score')
            seen.add(identity)
            p_group = p_group * float(reads['p_misaligned'][r])
            for position, letter, quality in observations(reads, r, positions):
                if quality > 40:
                    saw('quality above 40')
                if position in per_position and per_position[position][0] != rank:
                    saw('position seen by two reads')
                _rank, products = per_position.setdefault(position, (rank, {}))
                products[letter] = products.get(letter, 1.0) * float(table[min(quality, 40)])
            rank += 1
        calls = []
        for position, (first_rank, products) in per_position.items():
            if len(products) > 1:
                best = min(products.values())
                products = {letter: p for letter, p in products.items() if p <= best * 1000}
                saw('conflict resolved' if len(products) == 1 else 'conflict drops the position')
            if len(products) == 1:
                (letter, p), = products.items()
                if letter == ord('N'):
                    saw('N call')
                calls.append((first_rank, position, BASE_CODE[letter], p))
        if not calls:
            if per_position:
                saw('molecule with every position dropped')
            continue
        calls.sort(key=lambda c: c[:2])
        for _rank, position, code, p in calls:
            snp_calls.append((len(molecules), position, code, p))
        molecules.append((cb, ub, p_group))
    return np.array(molecules, dtype=MOLECULE_DTYPE).reshape(-1), np.array(snp_calls, dtype=SNP_CALL_DTYPE).reshape(-1)


REQUIRED_CASES = ('insertion', 'deletion', 'N-skip', 'leading soft clip', 'trailing soft clip', 'trailing hard clip',
                  'key split into molecules', 'event inside a molecule', 'complete duplicate', 'same span, other alignment score',
                  'conflict resolved', 'conflict drops the position', 'molecule with every position dropped', 'N call',
                  'quality above 40', 'position seen by two reads')


def special_cases(reads, positions):
    """How often every case of REQUIRED_CASES occurs in the reads (CIGAR shapes) and in their counting (trace of count_reads)."""
    trace = {}
    count_reads(reads, positions, trace=trace)
    for r in range(len(reads['reference_start'])):
        ops = [op for op, _length in _ops(reads, r)]
        aligned = [i for i, op in enumerate(ops) if op in BOTH]
        for name, found in (('insertion', 1 in ops), ('deletion', 2 in ops), ('N-skip', 3 in ops),
                            ('leading soft clip', bool(ops) and ops[0] == 4),
                            ('trailing soft clip', bool(aligned) and 4 in ops[aligned[-1] + 1:]),
                            ('trailing hard clip', bool(ops) and ops[-1] == 5)):
            if found:
                trace[name] = trace.get(name, 0) + 1
    return trace
