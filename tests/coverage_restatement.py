"""Plain Python / numpy restatement of the coverage and candidate contracts (DESIGN.md "Coverage and candidates"; the
counterpart of count_reads_restatement.py): test code that the device path and the golden fixtures are compared with,
written for clarity - pysam's aligned pairs as a list per read, the filter as the reference's four lines."""
import numpy as np

BOTH, REFERENCE_ONLY, READ_ONLY, NEITHER = (0, 7, 8), (2, 3), (1, 4), (5, 6)  # pysam's get_aligned_pairs: H and P move nothing
ROW = {ord(letter): row for row, letter in enumerate('ACGT')}


class InvalidReads(ValueError):
    """What the C entry point answers with its invalid-argument status."""


def _ops(reads, r):
    begin, n = int(reads['cigar_begin'][r]), int(reads['n_cigar'][r])
    if n < 0 or begin < 0 or begin + n > len(reads['cigar']):
        raise InvalidReads(f'read {r}: cigar range outside the array')
    return [(int(c) & 0xF, int(c) >> 4) for c in reads['cigar'][begin:begin + n]]


def aligned_pairs(reads, r):
    """[(index in the read, reference position)] of read r: the pairs of pysam's get_aligned_pairs(matches_only=True)."""
    pairs = []
    q, ref = 0, int(reads['reference_start'][r])
    for op, length in _ops(reads, r):
        if op in BOTH:
            pairs += [(q + k, ref + k) for k in range(length)]
            q, ref = q + length, ref + length
        elif op in REFERENCE_ONLY:
            ref += length
        elif op in READ_ONLY:
            q += length
        elif op not in NEITHER:
            raise InvalidReads(f'read {r}: CIGAR operation {op}')
    return pairs


def reference_end(reads, r):
    return int(reads['reference_start'][r]) + sum(length for op, length in _ops(reads, r) if op in BOTH + REFERENCE_ONLY)


def validate(reads):
    """The inputs the contract refuses, whatever the window."""
    starts = np.asarray(reads['reference_start'], dtype=np.int64)
    if np.any(np.diff(starts) < 0):
        raise InvalidReads('reference_start decreases')
    for r in range(len(starts)):
        seq_begin, l_seq = int(reads['seq_begin'][r]), int(reads['l_seq'][r])
        if l_seq < 0 or seq_begin < 0 or seq_begin + l_seq > len(reads['seq']):
            raise InvalidReads(f'read {r}: seq range outside the array')
        pairs = aligned_pairs(reads, r)
        if pairs and max(q for q, _ in pairs) >= l_seq:
            raise InvalidReads(f'read {r}: an aligned base beyond l_seq')
        if reference_end(reads, r) >= 2 ** 31:
            raise InvalidReads(f'read {r}: reference_end beyond 2^31 - 1')


def coverage(reads, start, stop, quality_threshold=15):
    """int32[4, stop - start], rows A, C, G, T; `reads` maps the names of DecodedReads to arrays."""
    validate(reads)
    counts = np.zeros((4, stop - start), dtype=np.int32)
    for r in range(len(reads['reference_start'])):
        seq_begin = int(reads['seq_begin'][r])
        for q, position in aligned_pairs(reads, r):
            if not start <= position < stop:
                continue
            if quality_threshold != 0 and int(reads['qual'][seq_begin + q]) < quality_threshold:
                continue
            row = ROW.get(int(reads['seq'][seq_begin + q]))
            if row is not None:
                counts[row, position - start] += 1
    return counts


def check_thresholds(minimum_coverage, minimum_alternative_fraction, minimum_alternative_coverage, minimum_fraction_of_ref_and_alt,
                     max_snp_candidates):
    for value in (minimum_coverage, minimum_alternative_fraction, minimum_alternative_coverage, minimum_fraction_of_ref_and_alt):
        if not np.isfinite(value):
            raise ValueError('a threshold is not finite')
    if minimum_coverage < 0 or minimum_alternative_coverage < 0 or max_snp_candidates < 1:
        raise ValueError('a threshold that lets the tail pick non-candidates')


def candidates(counts, start, *, minimum_coverage, minimum_alternative_fraction=0.01, minimum_alternative_coverage=100,
               max_snp_candidates=10000, minimum_fraction_of_ref_and_alt=0.98):
    """Ascending int32 absolute candidate positions of a counted window (snp_detection.py:44-57 of the reference, with the
    contract's tie rule and absolute positions)."""
    check_thresholds(minimum_coverage, minimum_alternative_fraction, minimum_alternative_coverage, minimum_fraction_of_ref_and_alt,
                     max_snp_candidates)
    counts = np.asarray(counts, dtype=np.int64)
    total = counts.sum(axis=0)
    ordered = np.sort(counts, axis=0)
    alt, ref = ordered[-2], ordered[-1]
    both = (ref + alt).astype(np.float64)
    is_candidate = both > float(minimum_coverage)
    is_candidate &= both > float(minimum_fraction_of_ref_and_alt) * total.astype(np.float64)
    is_candidate &= alt.astype(np.float64) > float(minimum_alternative_coverage)
    is_candidate &= alt.astype(np.float64) > ref.astype(np.float64) * float(minimum_alternative_fraction)
    found = np.flatnonzero(is_candidate)
    if len(found) > max_snp_candidates:
        # the largest alt; among equal alt at the cut the higher positions (the tail of a stable ascending order)
        order = sorted(found, key=lambda p: (alt[p], p))
        found = np.sort(np.asarray(order[-max_snp_candidates:], dtype=np.int64))
    return (found + start).astype(np.int32)


def fragments(length, step):
    """The reference's fragments of a chromosome (snp_detection.py:194-195)."""
    return [(start, min(start + step, length)) for start in range(0, length, step)]


def find_candidates(reads, length=None, *, max_fragment_step=10_000_000, quality_threshold=15, **thresholds):
    """Ascending candidate positions of one chromosome over all of its fragments."""
    n = len(reads['reference_start'])
    if n == 0:
        return np.zeros(0, dtype=np.int32)
    if length is None:
        length = max(0, max(reference_end(reads, r) for r in range(n)))
    found = [np.zeros(0, dtype=np.int32)]
    for start, stop in fragments(length, max_fragment_step):
        found.append(candidates(coverage(reads, start, stop, quality_threshold), start, **thresholds))
    return np.concatenate(found)


OPS = {'M': 0, 'I': 1, 'D': 2, 'N': 3, 'S': 4, 'H': 5, 'P': 6, '=': 7, 'X': 8}


def make_reads(rows):
    """DecodedReads arrays from [(reference_start, 'cigar like 3H 5M 2P 4M', letters, qualities)]; qualities a list or one
    number.  The other per-read columns hold values the coverage must not look at."""
    columns = {name: [] for name in ('reference_start', 'cigar_begin', 'n_cigar', 'seq_begin', 'l_seq')}
    cigar, seq, qual = [], [], []
    for start, text, letters, qualities in rows:
        ops = [(OPS[token[-1]], int(token[:-1])) for token in text.split()]
        if np.isscalar(qualities):
            qualities = [qualities] * len(letters)
        assert len(qualities) == len(letters)
        columns['reference_start'].append(start)
        columns['cigar_begin'].append(len(cigar))
        columns['n_cigar'].append(len(ops))
        columns['seq_begin'].append(len(seq))
        columns['l_seq'].append(len(letters))
        cigar += [(length << 4) | op for op, length in ops]
        seq += list(letters.encode('ascii'))
        qual += list(qualities)
    n = len(rows)
    return dict(reference_start=np.asarray(columns['reference_start'], dtype=np.int32),
                compressed_cb=np.full(n, -1, dtype=np.int32), compressed_ub=np.full(n, -7, dtype=np.int32),
                p_misaligned=np.full(n, np.nan), alignment_score=np.full(n, -99, dtype=np.int32),
                cigar_begin=np.asarray(columns['cigar_begin'], dtype=np.int64), n_cigar=np.asarray(columns['n_cigar'], dtype=np.int32),
                seq_begin=np.asarray(columns['seq_begin'], dtype=np.int64), l_seq=np.asarray(columns['l_seq'], dtype=np.int32),
                cigar=np.asarray(cigar, dtype=np.uint32), seq=np.asarray(seq, dtype=np.uint8), qual=np.asarray(qual, dtype=np.uint8))


def _expected(width, entries):
    out = np.zeros((4, width), dtype=np.int32)
    for letter, position, count in entries:
        out['ACGT'.index(letter), position] = count
    return out


# The coverage rules pinned by hand: (name, reads, start, stop, quality_threshold, expected int32[4, stop - start]).
# Every expected array is written out position by position, not computed.
HAND_TABLE = [
    # H first and last move nothing: the five bases sit at 10 .. 14
    ('hard clips first and last', [(10, '3H 5M 4H', 'ACGTA', 30)], 8, 18, 15,
     _expected(10, [('A', 2, 1), ('C', 3, 1), ('G', 4, 1), ('T', 5, 1), ('A', 6, 1)])),
    # P in the middle moves nothing: q goes on at 2, r at 22
    ('padding in the middle', [(20, '2M 3P 2M', 'ACGT', 30)], 20, 25, 15,
     _expected(5, [('A', 0, 1), ('C', 1, 1), ('G', 2, 1), ('T', 3, 1)])),
    # 2S 2M 1I 2M 2D 1M 3N 1= 1X : bases 2,3 -> 100,101; base 4 inserted; 5,6 -> 102,103; 104,105 deleted; 7 -> 106;
    # 107..109 skipped; 8 -> 110; 9 -> 111
    ('I D N S = X', [(100, '2S 2M 1I 2M 2D 1M 3N 1= 1X', 'TTACGGTCAG', 30)], 98, 114, 15,
     _expected(16, [('A', 2, 1), ('C', 3, 1), ('G', 4, 1), ('T', 5, 1), ('C', 8, 1), ('A', 12, 1), ('G', 13, 1)])),
    # N, lower case and other letters are not counted
    ('N and lower case', [(5, '6M', 'ANaC*T', 30)], 5, 11, 15,
     _expected(6, [('A', 0, 1), ('C', 3, 1), ('T', 5, 1)])),
    # qualities 14, 15, 16 at threshold 15: the first base is dropped
    ('qualities at the threshold', [(0, '3M', 'AAA', [14, 15, 16])], 0, 3, 15,
     _expected(3, [('A', 1, 1), ('A', 2, 1)])),
    # threshold 0 counts every quality, 0 included
    ('threshold 0', [(0, '3M', 'AAA', [14, 0, 16])], 0, 3, 0,
     _expected(3, [('A', 0, 1), ('A', 1, 1), ('A', 2, 1)])),
    # a read over both edges of the window [12, 15): bases 2, 3, 4 of ten
    ('straddling both edges', [(10, '10M', 'ACGTACGTAC', 30)], 12, 15, 15,
     _expected(3, [('G', 0, 1), ('T', 1, 1), ('A', 2, 1)])),
    # reads wholly before and wholly after the window, one that ends exactly at its start, one that starts exactly at its stop
    ('wholly outside', [(0, '5M', 'AAAAA', 30), (5, '5M', 'CCCCC', 30), (20, '5M', 'GGGGG', 30), (40, '5M', 'TTTTT', 30)], 10, 20, 15,
     _expected(10, [])),
    # two reads pile up; every read counts (same start, same everything: no duplicate removal)
    ('no duplicate removal', [(3, '2M', 'AC', 30), (3, '2M', 'AC', 30), (4, '1M', 'G', 30)], 0, 6, 15,
     _expected(6, [('A', 3, 2), ('C', 4, 2), ('G', 4, 1)])),
]
