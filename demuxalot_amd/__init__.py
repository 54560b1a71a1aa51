"""demuxalot_amd: MI355X-native implementation of demuxalot's Demultiplexer EM hot path.

Drop-in names of the reference package (demuxalot/__init__.py:3-7) that belong to the hot path:
"""
__version__ = '0.1.0'

from .utils import BarcodeHandler, calls_per_barcode, summarize_counted_SNPs
from .snp_counter import (CompressedSNPCalls, DecodedReads, ReadCounter, ResidentCalls, ResidentReads, count_snps_from_read_chunks,
                          count_snps_from_reads)
from .genotypes import ProbabilisticGenotypes
from .demux import Demultiplexer, DevicePosteriors, invalidate_resident
from .pools import DevicePooledPosteriors, PooledPosteriors
from .ambient import AmbientEstimate, DeviceJointAmbientPosteriors, JointAmbientPosteriors
from .doublet_shares import DoubletSharePosteriors, default_shares
from .snp_detection import (coverage_from_reads, detect_snps_positions_from_calls, detect_snps_positions_from_reads,
                            find_candidate_positions, select_snps_from_calls)

__all__ = ['BarcodeHandler', 'CompressedSNPCalls', 'ProbabilisticGenotypes', 'Demultiplexer', 'DevicePosteriors', 'PooledPosteriors', 'DevicePooledPosteriors', 'AmbientEstimate', 'JointAmbientPosteriors', 'DeviceJointAmbientPosteriors', 'DoubletSharePosteriors', 'default_shares', 'invalidate_resident',
           'detect_snps_positions_from_calls', 'select_snps_from_calls', 'DecodedReads', 'ResidentReads', 'ResidentCalls', 'calls_per_barcode', 'summarize_counted_SNPs', 'count_snps_from_reads', 'count_snps_from_read_chunks', 'ReadCounter', 'coverage_from_reads',
           'find_candidate_positions', 'detect_snps_positions_from_reads']
