"""What the hot path reads of the reference's BarcodeHandler (demuxalot/utils.py:60-77): the sorted barcode
list, which defines the row order of every output, the number of barcodes, and the barcode's row of a read
(get_barcode_index, which DecodedReads.from_reads calls).  RG handling stays with the reference's class, whose
instances are accepted unchanged everywhere."""

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
