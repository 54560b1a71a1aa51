"""What the hot path reads of the reference's BarcodeHandler (demuxalot/utils.py:60-77): the sorted barcode
list, which defines the row order of every output, the number of barcodes, and the barcode's row of a read
(get_barcode_index, which DecodedReads.from_reads calls).  RG handling stays with the reference's class, whose
instances are accepted unchanged everywhere.  And the two summaries of counted calls behind the reference's
summarize_counted_SNPs (demuxalot/utils.py:163-180), without its plots."""
import numpy as np

UB_MODULUS = 2147483629  # the prime the reference reduces its molecule-barcode hash by (demuxalot/utils.py:22)


def hash_string(s) -> int:
    """The int32 code of a molecule barcode (UB): its letters as digits of a base-5 number, modulo UB_MODULUS.
    The same value as the reference's hash_string, so that compressed_ub of both packages agree."""
    value = 0
    for letter in s:
        value = value * 5 + ord(letter)
    return value % UB_MODULUS


class BarcodeHandler:
    def __init__(self, barcodes, tag='CB'):
        assert not isinstance(barcodes, (str, bytes)), 'pass the list of barcodes, not a file name'
        self.tag = tag
        self.ordered_barcodes = sorted(barcodes)
        self.barcode2index = {barcode: row for row, barcode in enumerate(self.ordered_barcodes)}
        assert len(self.barcode2index) == len(self.ordered_barcodes), 'all passed barcodes should be unique'

    @property
    def n_barcodes(self):
        return len(self.ordered_barcodes)

    def get_barcode_index(self, read):
        """Row of the read's barcode (its `tag`), or None when the read has no such tag or the barcode is not listed."""
        if not read.has_tag(self.tag):
            return None
        return self.barcode2index.get(read.get_tag(self.tag), None)

    @classmethod
    def from_file(cls, path):
        """One barcode per line (the format of the reference's example_data/test_barcodes.csv)."""
        with open(path) as lines:
            return cls([line.strip() for line in lines if line.strip()])


def calls_per_barcode(snp_counts, n_barcodes):
    """The two counters of the reference's summarize_counted_SNPs (utils.py:168-180) as arrays over the barcodes' rows, summed over
    the chromosomes: (calls int64[n_barcodes]: SNP calls of the barcode's molecules, transcripts int64[n_barcodes]: its molecules).

    :param snp_counts: dict chromosome -> CompressedSNPCalls (numpy bincount on the host) or ResidentCalls (counted on the device,
        no record is downloaded); one kind per dict
    """
    from .snp_counter import split_call_sets
    n_barcodes = int(n_barcodes)
    calls, transcripts = np.zeros(n_barcodes, dtype=np.int64), np.zeros(n_barcodes, dtype=np.int64)
    resident = split_call_sets(snp_counts, 'snp_counts')
    for chromosome, counted in snp_counts.items():
        if resident:
            c, t = counted.barcode_counts(n_barcodes)
        else:
            cb = np.asarray(counted.molecules['compressed_cb'][:counted.n_molecules])
            if len(cb) and (cb.min() < 0 or cb.max() >= n_barcodes):
                raise ValueError(f'{chromosome!r}: compressed_cb outside [0, n_barcodes)')
            t = np.bincount(cb, minlength=n_barcodes)
            c = np.bincount(cb[counted.snp_calls['molecule_index'][:counted.n_snp_calls]], minlength=n_barcodes)
        calls += c
        transcripts += t
    return calls, transcripts


def summarize_counted_SNPs(snp_counts):
    """The per-chromosome records of the reference's summarize_counted_SNPs (utils.py:171-176) as a DataFrame: n_molecules and
    n_snp_calls, indexed and sorted by chromosome.  No plot; calls_per_barcode gives what the reference's histograms show.
    Takes host containers or ResidentCalls."""
    import pandas as pd
    records = [dict(chromosome=chromosome, n_molecules=int(counted.n_molecules), n_snp_calls=int(counted.n_snp_calls))
               for chromosome, counted in snp_counts.items()]
    frame = pd.DataFrame(records, columns=['chromosome', 'n_molecules', 'n_snp_calls'])
    return frame.set_index('chromosome').sort_index()
