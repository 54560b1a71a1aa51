"""The read filter for cellranger output, with the defaults of the reference's (demuxalot/cellranger_specific.py:13-36):
what DecodedReads.from_reads takes as `parse_read`."""
from .utils import hash_string


def parse_read(read, umi_tag='UB', nhits_tag='NH', score_tag='AS', score_diff_max=8, mapq_threshold=20,
               p_misaligned_default=0.01):
    """(p_misaligned, compressed_ub) of a read that is kept, None of one that is dropped: an alignment score more than
    score_diff_max - 1 below the read length, several hits, no molecule barcode, or a low mapping quality."""
    too_many_edits = read.get_tag(score_tag) <= len(read.seq) - score_diff_max
    if too_many_edits or read.get_tag(nhits_tag) > 1 or not read.has_tag(umi_tag) or read.mapq < mapq_threshold:
        return None
    return p_misaligned_default, hash_string(read.get_tag(umi_tag))
