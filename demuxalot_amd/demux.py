"""Demultiplexer: the reference's EM front-end (demuxalot/demux.py) over the MI355X kernels.

Same static-method surface, argument meaning, output conventions and assertion behaviour as the
reference class, so `from demuxalot_amd import Demultiplexer` can replace
`from demuxalot import Demultiplexer` behind an unchanged front-end (BAM scanning, genotype
import).  Inputs are duck-typed: the reference's own CompressedSNPCalls / ProbabilisticGenotypes /
BarcodeHandler objects work as well as this package's mirrors.

What runs where
  GPU (rocPRIM sorts/scans + HIP kernels, dmx_pack_and_set_problem): variant matching, de-duplication
             with float32 products in call order, CSR/CSC derivation -> demux.py:276-300, 332-365
             (the public pack_calls(), whose results are host arrays, uses the C++ host twin
             dmx_pack_calls_host, which also works without a GPU)
  GPU:        regularised prior betas (dmx_set_prior_betas)     -> demux.py:367-388
              (numpy twin `_prior_betas` only inside the host-side pack_calls())
  GPU (HIP):  beta -> probability normalisation                -> demux.py:267-274
              per-barcode log-likelihood accumulation + softmax -> demux.py:246-265, :101, :152
              squared-posterior beta update (+ RCCL all-reduce) -> demux.py:113-118
  GPU (HIP):  Demultiplexer.aggregate_on_snps = True: per-(barcode, SNP) regularised E-step over the molecule
              calls and the float64 M-step that follows it                   -> demux.py:204-244
There is no CPU fallback for the GPU steps.
"""
import contextlib
import os
from typing import Dict, NamedTuple, Tuple

import numpy as np
import pandas as pd

from . import _lib, donor_readout
from .ambient import (AmbientEstimate, DeviceJointAmbientPosteriors, JointAmbientPosteriors, assigned_donors, best_singlets, default_alphas, resolve_assignments,
                      resolve_fractions, resolve_grid)
from .device import (DeviceContext, acquire_private_context, default_device, get_context, release_private_context,
                     shared_context_lock)
from .doublet_shares import DoubletSharePosteriors, resolve_shares
from .pools import DevicePooledPosteriors, PooledPosteriors, resolve_pools

_MOLECULE_CALL_DTYPE = [('variant_id', 'int32'), ('snp_id', 'int32'), ('compressed_cb', 'int32'),
                        ('molecule_id', 'int32'), ('p_base_wrong', 'float32'), ('p_molecule_aligned_wrong', 'float32')]
_BASES = {'A': 0, 'C': 1, 'G': 2, 'T': 3, 'N': 4}
_BASE_TABLE = np.full(256, 255, dtype=np.uint8)
for _letter, _code in _BASES.items():
    _BASE_TABLE[ord(_letter)] = _code


class _Packed:
    """Result of the host-side repack: what the device needs plus what pack_calls returns."""
    __slots__ = ('v2snp', 'betas', 'variant_id', 'compressed_cb', 'p_base_wrong', 'variant_count',
                 'molecule_calls', 'n_molecule_calls')


_UNSET = object()


def _variant_keys(genotypes, columns=_UNSET):
    """var2varid -> per-row key arrays (chromosome index, position, base code) and the chromosome numbering.
    `columns`: variant_columns(genotypes.var2varid) when the caller has them already."""
    from .genotypes import variant_columns
    n_variants = genotypes.n_variants
    if columns is _UNSET:
        columns = variant_columns(genotypes.var2varid)
    base_codes = None
    if columns is not None:
        rows, chrom_codes, chrom_names, pos, bases = columns
        try:  # single-letter bases: one join + a 256-entry table instead of a dict lookup per variant
            letters = np.frombuffer(''.join(bases).encode('ascii'), dtype=np.uint8)
            if len(letters) == len(rows):
                base_codes = _BASE_TABLE[letters]
        except (TypeError, UnicodeEncodeError):
            base_codes = None
    if base_codes is not None and (base_codes < 255).all() and (len(pos) == 0 or pos.max() < 2 ** 31):
        assert len(rows) == n_variants and (len(rows) == 0 or (rows.min() >= 0 and rows.max() < n_variants)), \
            'var2varid rows must enumerate 0..n_variants-1'
        seen = np.zeros(n_variants, dtype=bool)
        seen[rows] = True
        assert seen.all(), 'var2varid rows must enumerate 0..n_variants-1'  # demux.py:317 (a repeated row leaves a gap)
        var_chrom = np.zeros(n_variants, dtype=np.int32)
        var_pos = np.zeros(n_variants, dtype=np.int32)
        var_base = np.zeros(n_variants, dtype=np.uint8)
        var_chrom[rows] = chrom_codes
        var_pos[rows] = pos
        var_base[rows] = base_codes
        return (var_chrom, var_pos, var_base), {name: i for i, name in enumerate(chrom_names)}
    chrom_index = {}
    var_chrom = np.zeros(n_variants, dtype=np.int32)
    var_pos = np.zeros(n_variants, dtype=np.int32)
    var_base = np.zeros(n_variants, dtype=np.uint8)
    seen = np.zeros(n_variants, dtype=bool)
    for (chrom, pos, base), row in genotypes.var2varid.items():
        assert 0 <= row < n_variants and not seen[row], 'var2varid rows must enumerate 0..n_variants-1'
        seen[row] = True
        var_chrom[row] = chrom_index.setdefault(chrom, len(chrom_index))
        var_pos[row] = pos
        var_base[row] = _BASES[base]
    assert seen.all(), 'var2varid rows must enumerate 0..n_variants-1'  # demux.py:317
    return (var_chrom, var_pos, var_base), chrom_index


def _var2varid_fingerprint(var2varid):
    """Identity of a (chrom, pos, base) -> row dict cheap enough to take on every call: the object, its length, its first
    and last entries and ~61 entries at a stride (dicts keep insertion order and the importers only ever append:
    genotypes.py extend_variants; the mutators of demuxalot_amd.ProbabilisticGenotypes drop the kept arrays themselves)."""
    n = len(var2varid)
    if n == 0:
        return id(var2varid), 0
    import itertools
    sample = tuple(itertools.islice(var2varid.items(), 0, None, max(1, n // 61)))  # (a walk at C speed: ~1 ms for 200k entries)
    return id(var2varid), n, next(reversed(var2varid.items())), hash(sample)


def _cached_variant_keys(genotypes):
    """(fingerprint, v2snp, (var_chrom, var_pos, var_base), chromosome -> index) of a genotypes object.  Walking var2varid is
    30 ms for 200k variants - a third of a predict_posteriors call on 78 M calls - and predict -> learn -> predict on the
    same genotypes (examples/2-with-detection-of-new-SNPs.ipynb cells 12 / 16-18, tests/test_synthetic.py:184-190) walked it
    every time: the arrays are kept on the object, keyed by the fingerprint of its var2varid (assigning another dict, or
    adding variants, invalidates them).  A mapping edited in place at unchanged length, first and last entry is not
    detected: set `genotypes._amd_variant_keys = None` after such surgery."""
    from .genotypes import ProbabilisticGenotypes, snp_ids_from_columns, variant_columns
    own_numbering = getattr(type(genotypes), 'get_snp_ids_for_variants', None) is ProbabilisticGenotypes.get_snp_ids_for_variants
    fingerprint = (_var2varid_fingerprint(genotypes.var2varid), genotypes.n_variants, own_numbering)
    cached = getattr(genotypes, '_amd_variant_keys', None)
    if cached is not None and cached[0] == fingerprint:
        return cached
    columns = variant_columns(genotypes.var2varid)  # one walk of var2varid for the SNP numbering and the row keys
    if own_numbering and columns is not None:
        v2snp = snp_ids_from_columns(columns)
    else:
        v2snp = genotypes.get_snp_ids_for_variants()
    assert np.all(v2snp >= 0)
    keys, chrom_index = _variant_keys(genotypes, columns)
    cached = (fingerprint, v2snp, keys, chrom_index)
    try:
        genotypes._amd_variant_keys = cached
    except AttributeError:  # an object that takes no attributes: nothing is kept
        pass
    return cached


def _sampled_checksum(records):
    """crc32 of the head, the tail and ~512 strided records of a record array.  NOT what the resident problem is keyed by any more
    (a sparse in-place edit slips through): kept for DEMUXALOT_AMD_RESIDENT=sampled, the opt-in of callers who never edit their
    containers in place and want the last 15 ms of a repeated call."""
    import zlib
    n = len(records)
    if n == 0:
        return 0
    flat = np.ascontiguousarray(records).view(np.uint8).reshape(-1)
    crc = zlib.crc32(flat[:4096].tobytes())
    crc = zlib.crc32(flat[-4096:].tobytes(), crc)
    return zlib.crc32(np.ascontiguousarray(records[::max(1, n // 512)]).view(np.uint8).tobytes(), crc)


def _content_hash(records):
    """64-bit hash of EVERY byte of a record array (dmx_hash_host: several host threads, memory bandwidth - 2 GB in ~15 ms).
    The reference packs its inputs anew on every call (demux.py:303); a packed problem of an earlier call stands in for that
    only when every record of every container hashes as it did then, whatever object the records live in."""
    import ctypes
    records = np.ascontiguousarray(records)
    out = ctypes.c_uint64(0)
    _lib.check(_lib.load().dmx_hash_host(records.ctypes.data if records.size else None, int(records.nbytes), 0, ctypes.byref(out)))
    return int(out.value)


def resident_policy():
    """DEMUXALOT_AMD_RESIDENT = full (default: reuse keyed by the content hash of every record) | sampled (identity + a
    sampled checksum, round 5's key: in-place edits of single records are NOT seen) | 0 (never reuse: every call packs)."""
    policy = os.environ.get('DEMUXALOT_AMD_RESIDENT', 'full').lower()
    policy = {'1': 'full', 'on': 'full', 'off': '0', 'never': '0', 'none': '0'}.get(policy, policy)
    assert policy in ('full', 'sampled', '0'), f'DEMUXALOT_AMD_RESIDENT={policy!r}: full, sampled or 0'
    return policy


def invalidate_resident(genotypes=None, barcode_handler=None):
    """Forget what the front-end keeps between calls: the packed problem resident on the shared device context(s) and, when
    given, the key arrays kept on a genotypes object and the Index kept on a barcode handler.  The next call packs anew, as
    every call of the reference does."""
    from . import device
    with device.shared_context_lock:
        for ctx in device.shared_contexts():
            ctx._resident_key = None
    if genotypes is not None:
        try:
            genotypes._amd_variant_keys = None
        except AttributeError:
            pass
    if barcode_handler is not None:
        try:
            barcode_handler._amd_index = None
        except AttributeError:
            pass


def _flatten_inputs(chromosome2compressed_snp_calls, genotypes, want_molecule_table):
    """var2varid -> per-row key arrays; per-chromosome call containers -> flat call arrays."""
    (var_chrom, var_pos, var_base), chrom_index = _variant_keys(genotypes)

    parts = []
    n_expected = n_taken = 0
    for chrom, container in chromosome2compressed_snp_calls.items():
        n = container.n_snp_calls
        n_expected += n
        if chrom not in chrom_index:
            continue  # demux.py:339-341: no SNPs on this chromosome (the cursor is not advanced)
        calls = container.snp_calls[:n]
        molecules = container.molecules[:container.n_molecules]
        mol = calls['molecule_index']
        part = dict(chrom=np.full(n, chrom_index[chrom], dtype=np.int32), pos=calls['snp_position'],
                    base=calls['base_index'], cb=molecules['compressed_cb'][mol], p=calls['p_base_wrong'])
        if want_molecule_table:
            part['mol'] = mol
            part['pmis'] = molecules['p_group_misaligned'][mol]
        parts.append(part)
        n_taken += n
    assert n_taken == n_expected  # demux.py:359 (fires when a chromosome with calls has no variants)

    def cat(name, dtype):
        if not parts:
            return np.zeros(0, dtype=dtype)
        return np.ascontiguousarray(np.concatenate([p[name] for p in parts]), dtype=dtype)

    flat = dict(chrom=cat('chrom', np.int32), pos=cat('pos', np.int32), base=cat('base', np.uint8),
                cb=cat('cb', np.int32), p=cat('p', np.float32))
    if want_molecule_table:
        flat['mol'] = cat('mol', np.int32)
        flat['pmis'] = cat('pmis', np.float32)
    return (var_chrom, var_pos, var_base), flat


def _prior_betas(genotypes, v2snp, mol_per_variant, add_data_prior):
    """demux.py:367-388. beta' = beta + f32((1 + [data] n_mol/(n_mol_snp + 100)
    + betasum/(betasum_snp + 100)) * default_prior)[:, None]; float64 per-SNP sums."""
    betas = genotypes.get_betas()
    assert np.all(betas >= 0), 'bad genotypes provided, negative betas appeared'

    def share_within_snp(per_variant, regularization):
        assert len(per_variant) == len(v2snp)
        per_snp = np.bincount(v2snp, weights=per_variant)[v2snp] if len(v2snp) else np.zeros(0)
        return per_variant / (per_snp + regularization)

    scale = 1.
    if add_data_prior:
        scale = scale + share_within_snp(mol_per_variant, 100.)
    scale = scale + share_within_snp(betas.sum(axis=1), 100.)
    addition = scale[:, np.newaxis] * genotypes.default_prior
    out = betas + addition.astype(betas.dtype)
    out.flags.writeable = False
    return out


def _pack(chromosome2compressed_snp_calls, genotypes, add_data_prior, want_molecule_table=False) -> _Packed:
    lib = _lib.load()
    (var_chrom, var_pos, var_base), flat = _flatten_inputs(
        chromosome2compressed_snp_calls, genotypes, want_molecule_table)
    v2snp = genotypes.get_snp_ids_for_variants()
    assert np.all(v2snp >= 0)
    n_variants, n_calls = len(var_pos), len(flat['pos'])

    call_variant = np.empty(n_calls, dtype=np.int32) if want_molecule_table else None
    out_variant = np.empty(n_calls, dtype=np.int32)
    out_cb = np.empty(n_calls, dtype=np.int32)
    out_p = np.empty(n_calls, dtype=np.float32)
    out_count = np.empty(n_calls, dtype=np.int64)
    mol_per_variant = np.zeros(n_variants, dtype=np.int64)
    import ctypes
    n_matched, n_unique = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(lib.dmx_pack_calls_host(
        n_variants, _lib.ptr(var_chrom), _lib.ptr(var_pos), _lib.ptr(var_base),
        n_calls, _lib.ptr(flat['chrom']), _lib.ptr(flat['pos']), _lib.ptr(flat['base']), _lib.ptr(flat['cb']),
        _lib.ptr(flat['p']), _lib.ptr(call_variant), ctypes.byref(n_matched), ctypes.byref(n_unique),
        _lib.ptr(out_variant), _lib.ptr(out_cb), _lib.ptr(out_p), _lib.ptr(out_count), _lib.ptr(mol_per_variant)))
    n = n_unique.value

    packed = _Packed()
    packed.v2snp = v2snp
    packed.variant_id = out_variant[:n].copy()
    packed.compressed_cb = out_cb[:n].copy()
    packed.p_base_wrong = out_p[:n].copy()
    packed.variant_count = out_count[:n].copy()
    packed.n_molecule_calls = n_matched.value
    packed.betas = _prior_betas(genotypes, v2snp, mol_per_variant, add_data_prior)
    packed.molecule_calls = None
    if want_molecule_table:
        keep = call_variant != -1
        table = np.zeros(int(keep.sum()), dtype=_MOLECULE_CALL_DTYPE)
        table['variant_id'] = call_variant[keep]
        table['snp_id'] = v2snp[call_variant[keep]]
        table['compressed_cb'] = flat['cb'][keep]
        table['molecule_id'] = flat['mol'][keep]
        table['p_base_wrong'] = flat['p'][keep]
        table['p_molecule_aligned_wrong'] = flat['pmis'][keep]
        packed.molecule_calls = table
    return packed


def _pack_on_device(chromosome2compressed_snp_calls, genotypes, n_barcodes, add_data_prior, fetch_betas=True, ctx=None,
                    reduce_molecule_counts=None):
    """The repack of predict / learn, on the GPU: flattening of the containers' records, matching +
    de-duplication + layout derivation (dmx_pack_containers_and_set_problem) and the regularised prior betas
    (dmx_set_prior_betas).
    Returns (ctx with the problem and betas resident, regularised prior betas).  `ctx` None = the shared cached
    context (the caller holds shared_context_lock).  `reduce_molecule_counts` (barcode-sharded runs): maps this
    shard's molecule counts per variant to the counts of the whole experiment, which the data term of the
    prior is made of (demux.py:381-384)."""
    from .snp_counter import MOLECULE_DTYPE, SNP_CALL_DTYPE, split_call_sets
    if ctx is None:
        ctx = get_context()
    shared = bool(getattr(ctx, '_is_shared', False))  # the process-wide context (its users hold shared_context_lock)
    if split_call_sets(chromosome2compressed_snp_calls):
        return _pack_resident_calls(ctx, shared, chromosome2compressed_snp_calls, genotypes, n_barcodes, add_data_prior, fetch_betas,
                                    reduce_molecule_counts)
    containers = list(chromosome2compressed_snp_calls.values())
    raw = all(c.snp_calls.dtype == SNP_CALL_DTYPE and c.molecules.dtype == MOLECULE_DTYPE for c in containers)
    # The packed problem stays resident on the shared context: predict_posteriors followed by learn_genotypes on the same
    # containers and genotypes (the reference's own usage pattern, see _cached_variant_keys) packs once.  Key: the content
    # hash of EVERY record of every container (no object identities: an array edited in place hashes differently, a freed
    # id() that comes back means nothing), the fingerprint of var2varid, the shape.  resident_policy(): the switch.
    # The full hashes cost 16 ms for 2 GB of records: on a call whose inputs CANNOT be the resident ones (other shapes, or a sampled
    # checksum that already differs) they are taken in a second thread BEHIND the upload - next to it they competed with the runtime's
    # own host copies for memory bandwidth: 91 instead of 77 ms - while the device packs (13 ms) and computes the prior, and are joined
    # before this function returns (the caller may edit its arrays after that); only a call that looks like a repeat pays for them
    # up front - and saves the 45 ms upload and the 13 ms device pack when they confirm it.
    key = None
    hashes_later = None   # thread computing the full hashes of a call that packs (policy 'full')
    policy = resident_policy() if (shared and raw and reduce_molecule_counts is None) else '0'
    resident = getattr(ctx, '_resident_key', None)
    named = list(chromosome2compressed_snp_calls.items())

    def full_hashes():
        return tuple((_content_hash(c.snp_calls[:c.n_snp_calls]), _content_hash(c.molecules[:c.n_molecules])) for _chrom, c in named)

    if policy == 'full':
        meta = (tuple((chrom, int(c.n_snp_calls), int(c.n_molecules)) for chrom, c in named),
                _var2varid_fingerprint(genotypes.var2varid), genotypes.n_variants, genotypes.n_genotypes, int(n_barcodes),
                bool(getattr(ctx, '_keep_molecule_calls', False)))
        sampled = tuple((_sampled_checksum(c.snp_calls[:c.n_snp_calls]), _sampled_checksum(c.molecules[:c.n_molecules])) for _chrom, c in named)
        if resident is not None and resident[:3] == ('full', meta, sampled):
            key = ('full', meta, sampled, full_hashes())   # looks like a repeat: every record decides
        else:
            import threading
            box = []
            hashes_later = (threading.Thread(target=lambda: box.append(full_hashes())), box, meta, sampled)
    elif policy == 'sampled':
        key = ('sampled', tuple((chrom, id(c.snp_calls), id(c.molecules), int(c.n_snp_calls), int(c.n_molecules),
                                 _sampled_checksum(c.snp_calls[:c.n_snp_calls]), _sampled_checksum(c.molecules[:c.n_molecules]))
                                for chrom, c in named),
               _var2varid_fingerprint(genotypes.var2varid), genotypes.n_variants, genotypes.n_genotypes, int(n_barcodes),
               bool(getattr(ctx, '_keep_molecule_calls', False)))
    if key is not None and resident == key:
        molecules = None  # (the counts per variant are on the device: dmx_set_prior_betas takes them from there)
    elif raw:
        # The containers' packed records go to the GPU as they are and are taken apart there - and they go FIRST, in a
        # second thread (the upload is one foreign call, which releases the interpreter), while this one walks
        # var2varid: 45 ms of upload next to 30 ms of walk for 78.65 M calls and 200 k variants.
        import threading
        items = list(chromosome2compressed_snp_calls.items())
        staged = [(k, container.snp_calls[:container.n_snp_calls], container.molecules[:container.n_molecules])
                  for k, (_chrom, container) in enumerate(items)]
        failure = []

        def stage():
            try:
                ctx.stage_containers(staged)
            except BaseException as exc:  # noqa: BLE001 - re-raised below, on the calling thread
                failure.append(exc)

        worker = threading.Thread(target=stage)
        worker.start()
        try:
            _fp, v2snp, (var_chrom, var_pos, var_base), chrom_index = _cached_variant_keys(genotypes)
        except BaseException:
            worker.join()
            if not failure:  # the worker did stage them (~17 bytes per call on the GPU): give them back before unwinding
                try:
                    ctx.release_problem()
                except Exception:  # noqa: BLE001
                    pass
            raise
        worker.join()
        if failure:
            raise failure[0]
        if hashes_later is not None:
            hashes_later[0].start()   # (the records are on the device: the host's memory system is free for the hashes)
        chrom_of_container = []
        for chrom, container in items:
            if chrom not in chrom_index:  # demux.py:339-341, 359: calls on a chromosome without variants trip the reference's final assert
                assert container.n_snp_calls == 0
            chrom_of_container.append(chrom_index.get(chrom, -1))
        try:
            _m, _u, molecules = ctx.pack_staged_and_set_problem(n_barcodes, genotypes.n_genotypes, var_chrom, var_pos, var_base, v2snp,
                                                                chrom_of_container)
        except BaseException:
            if hashes_later is not None:
                hashes_later[0].join()
            raise
        ctx._resident_key = key   # (policy 'full': set below, once the hashes are in)
    else:
        v2snp = genotypes.get_snp_ids_for_variants()
        assert np.all(v2snp >= 0)
        (var_chrom, var_pos, var_base), flat = _flatten_inputs(chromosome2compressed_snp_calls, genotypes, False)
        _m, _u, molecules = ctx.pack_and_set_problem(n_barcodes, genotypes.n_genotypes, var_chrom, var_pos, var_base, v2snp,
                                                     flat['chrom'], flat['pos'], flat['base'], flat['cb'], flat['p'])
    # regularised prior on the GPU too (a single rank's molecule counts per variant stay on the device)
    if reduce_molecule_counts is not None and add_data_prior:
        molecules = reduce_molecule_counts(molecules)
    else:
        molecules = None
    try:
        betas = ctx.set_prior_betas(genotypes.get_betas(), genotypes.default_prior, add_data_prior,
                                    mol_per_variant=molecules, fetch=fetch_betas)
    finally:
        if hashes_later is not None and hashes_later[0].ident is not None:   # (started: the records went to the device)
            thread, box, meta, sampled = hashes_later
            thread.join()
            ctx._resident_key = ('full', meta, sampled, box[0]) if box else None   # (a hash that failed: nothing is kept)
    return ctx, betas


def _resident_calls_key(named, genotypes, n_barcodes, keep_molecule_calls):
    """What a problem packed from ResidentCalls is kept under on the shared context.  named: [(chromosome, ResidentCalls)].  No
    record is looked at: a handle is never reused and a sealed set never changes, so (chromosome, handle) is exact."""
    return ('resident-calls', tuple((chrom, int(calls._handle)) for chrom, calls in named), _var2varid_fingerprint(genotypes.var2varid),
            genotypes.n_variants, genotypes.n_genotypes, int(n_barcodes), bool(keep_molecule_calls))


def _pack_resident_calls(ctx, shared, chromosome2resident_calls, genotypes, n_barcodes, add_data_prior, fetch_betas, reduce_molecule_counts):
    """_pack_on_device for a dict of ResidentCalls (snp_counter.py): the sets' device views are staged where the host path uploads
    the records - no call record crosses the link, none is read on the host - and the rest is the host path's.  The sets may live
    on another context of ctx's device.  The resident key on the shared context needs no hash: handles are never reused and a
    sealed set never changes, so (chromosome, handle) names the records exactly."""
    named = list(chromosome2resident_calls.items())
    views = [(k, calls._view(ctx.device)) for k, (_chrom, calls) in enumerate(named)]  # (a closed set raises here, before any reuse)
    key = None
    if shared and reduce_molecule_counts is None and resident_policy() != '0':
        key = _resident_calls_key(named, genotypes, n_barcodes, getattr(ctx, '_keep_molecule_calls', False))
    if key is not None and getattr(ctx, '_resident_key', None) == key:
        molecules = None  # (the counts per variant are on the device: dmx_set_prior_betas takes them from there)
    else:
        ctx.stage_device_containers(views)
        try:
            _fp, v2snp, (var_chrom, var_pos, var_base), chrom_index = _cached_variant_keys(genotypes)
            chrom_of_container = []
            for chrom, calls in named:
                if chrom not in chrom_index:  # demux.py:339-341, 359: calls on a chromosome without variants trip the reference's final assert
                    assert calls.n_snp_calls == 0
                chrom_of_container.append(chrom_index.get(chrom, -1))
        except BaseException:
            try:  # the staged calls (~17 bytes per call on the GPU) go back before unwinding
                ctx.release_problem()
            except Exception:  # noqa: BLE001
                pass
            raise
        _m, _u, molecules = ctx.pack_staged_and_set_problem(n_barcodes, genotypes.n_genotypes, var_chrom, var_pos, var_base, v2snp,
                                                            chrom_of_container)
        ctx._resident_key = key
    if reduce_molecule_counts is not None and add_data_prior:
        molecules = reduce_molecule_counts(molecules)
    else:
        molecules = None
    betas = ctx.set_prior_betas(genotypes.get_betas(), genotypes.default_prior, add_data_prior, mol_per_variant=molecules, fetch=fetch_betas)
    return ctx, betas


def _barcode_index(barcode_handler, name=None):
    """pd.Index of barcode_handler.ordered_barcodes (200k strings: ~4 ms to build, per frame), kept on the handler and
    shared by the frames of later calls (an Index is immutable; every frame gets its own shallow copy with its name)."""
    barcodes = barcode_handler.ordered_barcodes
    fingerprint = (id(barcodes), len(barcodes), barcodes[0] if len(barcodes) else None, barcodes[-1] if len(barcodes) else None)
    cached = getattr(barcode_handler, '_amd_index', None)
    if cached is None or cached[0] != fingerprint:
        cached = (fingerprint, pd.Index(list(barcodes)))
        try:
            barcode_handler._amd_index = cached
        except AttributeError:
            pass
    index = cached[1].copy()
    index.name = name
    return index


def _option_names(genotype_names, doublet_prior):
    """Column names: singlets, then 'A+B' for A before B (demux.py:175-191)."""
    names = list(genotype_names)
    if doublet_prior != 0:
        assert doublet_prior > 0
        names = names + [f'{a}+{b}' for i, a in enumerate(genotype_names) for b in genotype_names[i + 1:]]
    return names


def _release_pooled_context(ctx):
    """close() of a DevicePooledPosteriors: the private context goes back to its pool as it came (the switch off, the slot dropped
    with the problem)."""
    ctx.set_keep_pooled(False)
    release_private_context(ctx)


@contextlib.contextmanager
def _generator_context():
    """The private context of a staged generator, for the generator's life: it goes back to its pool when the generator ends or
    its consumer stops early (GeneratorExit: nothing wrong with the context), and as failed on any other exception."""
    ctx = acquire_private_context()
    try:
        yield ctx
    except BaseException as error:
        release_private_context(ctx, failed=not isinstance(error, GeneratorExit))
        raise
    release_private_context(ctx)


@contextlib.contextmanager
def _handed_over_context():
    """A private context that the result of the call keeps (on_device=True): closed when the call fails, left open when it succeeds -
    the result object gives it back."""
    ctx = acquire_private_context()
    try:
        yield ctx
    except BaseException:
        ctx.close()
        raise


class _PoolSetup(NamedTuple):
    """What a pooled pass and the framing of its result need to know of the pools: one description for "pools given" and for the one
    pool of everybody that stands in without them."""
    pooled: bool                  # the caller gave pools: the result is a PooledPosteriors; False: frames over the one pool
    pool_names: list              # ['all'] without pools
    pool_columns: list            # per pool the ascending table columns of its donors
    pool_of_barcode: np.ndarray   # int32[B], -1: in no pool
    option_names: list            # per pool the names of its options
    pair_penalty: np.ndarray      # float32[n_pools]: the reference's bonus for the pool's genotype list (demux.py:164-169: the prior
                                  # doublet share is doublet_prior inside every pool), 0.0 for a pool of one donor


def _pool_setup(genotypes, barcode_handler, doublet_prior, barcode2pool, pool2donors, who):
    """The _PoolSetup of an entry point.  With barcode2pool / pool2donors: the pools as resolve_pools reads them (its ValueErrors).
    Without them: one pool that scores every barcode against all donors with the reference's penalties; `who` names the entry in the
    ValueError for more options than one pool holds.  who=None: an entry that takes pools only."""
    names = list(genotypes.genotype_names)
    pooled = who is None or barcode2pool is not None
    if pooled:
        pool_names, pool_columns, pool_of_barcode = resolve_pools(names, barcode_handler.ordered_barcodes, barcode2pool, pool2donors)
    else:
        G = genotypes.n_genotypes
        n_options = G * (G + 1) // 2 if doublet_prior != 0 else G
        if n_options > 1024:
            raise ValueError(f'{who}: {G} donors make {n_options} options, more than the 1024 one pool can hold (44 donors with doublets); '
                             'give every barcode a pool of its own donors with barcode2pool / pool2donors')
        pool_names, pool_columns = ['all'], [np.arange(G, dtype=np.int64)]
        pool_of_barcode = np.zeros(barcode_handler.n_barcodes, dtype=np.int32)
    option_names = [_option_names([names[g] for g in columns], doublet_prior) for columns in pool_columns]
    pair_penalty = np.array([Demultiplexer._doublet_penalties(len(columns), doublet_prior)[-1] if len(columns) > 1 else 0.0
                             for columns in pool_columns], dtype=np.float32)
    return _PoolSetup(pooled, pool_names, pool_columns, pool_of_barcode, option_names, pair_penalty)


def _framed_posteriors(setup, barcode_handler, out, index_name):
    """The result of a pooled pass (its dict `out`) as the entry points return it: with pools a PooledPosteriors; without, the frames
    of the one pool with predict_posteriors' index and columns - (logits_df, probs_df), or probs_df alone when the logits were not
    fetched.  index_name: the frames' (a PooledPosteriors names its own 'BARCODE')."""
    if setup.pooled:
        return PooledPosteriors(barcode_handler.ordered_barcodes, setup.pool_names, setup.option_names, setup.pool_of_barcode, out['row_ptr'],
                                out['logits'], out['probs'], out['best_option'], out['best_prob'], out['doublet_mass'])
    columns = setup.option_names[0]
    shape = (barcode_handler.n_barcodes, len(columns))
    frames = tuple(pd.DataFrame(data=out[what].reshape(shape), index=_barcode_index(barcode_handler, index_name), columns=columns)
                   for what in ('logits', 'probs') if out[what] is not None)
    return frames if len(frames) == 2 else frames[0]


def _set_up_table(ctx, chromosome2compressed_snp_calls, genotypes, n_barcodes, p_genotype_clip):
    """What every one-pass entry does before its pass: the calls packed on the context (prior betas without the data term), no
    addition, the genotype table of the P-step - which must be finite."""
    _pack_on_device(chromosome2compressed_snp_calls, genotypes, n_barcodes, False, fetch_betas=False, ctx=ctx)
    ctx.set_addition(None)
    genotype_prob = ctx.probs_from_betas(p_genotype_clip)
    assert np.isfinite(genotype_prob).all()


def _pooled_on_device(run, barcode_handler, setup):
    """run(ctx) - pack, table and one pooled pass with nothing of the rows fetched - on a private context with the keep switch on:
    (the pass's dict, the DevicePooledPosteriors over the slot it left)."""
    with _handed_over_context() as ctx:
        ctx.set_keep_pooled(True)
        out = run(ctx)
        posteriors = DevicePooledPosteriors(ctx, barcode_handler.ordered_barcodes, setup.pool_names, setup.option_names,
                                            [len(c) for c in setup.pool_columns], setup.pool_of_barcode, out['row_ptr'], out['best_option'],
                                            out['best_prob'], out['doublet_mass'], index_name='BARCODE', release=_release_pooled_context)
    return out, posteriors


class DevicePosteriors:
    """Posteriors (and logits) of one predict_posteriors / learn_genotypes call, kept on the GPU
    (`on_device=True`), with the reductions users of the reference apply to the DataFrame done there:
    nothing of size [B, K] crosses PCIe unless to_dataframes() / rows() ask for it.
    Owns a private device context; close() (or garbage collection) hands it back to a small pool with the problem
    released into the context's block cache - parked, re-used by the next call, and returned to the driver by
    demuxalot_amd.device.trim_device_caches() or by any allocation that would otherwise run out of device memory."""

    def __init__(self, ctx, barcodes, column_names, index_name=None, pooled=True, n_donors=None):
        self._ctx = ctx
        self.n_donors = int(ctx.G if n_donors is None else n_donors)  # the singlet columns are the first n_donors
        self._pooled = pooled  # False: a context set up elsewhere (e.g. with a communicator attached): destroyed on close
        self.barcodes = list(barcodes)
        self.columns = list(column_names)
        self.index_name = index_name

    @property
    def shape(self):
        return len(self.barcodes), len(self.columns)

    def _index(self, barcodes=None):
        index = pd.Index(self.barcodes if barcodes is None else barcodes)
        index.name = self.index_name
        return index

    def assignments(self, threshold=0.9) -> pd.Series:
        """probs[probs.max(axis=1).gt(threshold)].idxmax(axis=1)
        (examples/2-with-detection-of-new-SNPs.ipynb cell 14; snp_detection.py:166)."""
        best, _prob, _n = self._ctx.get_assignments_above(threshold)
        rows = np.flatnonzero(best >= 0)
        names = np.asarray(self.columns, dtype=object)[best[rows]]
        return pd.Series(names, index=self._index([self.barcodes[i] for i in rows]))

    def best(self) -> pd.DataFrame:
        """Per barcode: the most probable option and its posterior (idxmax / max of every row); None / NaN for a row
        without any non-NaN posterior."""
        best, prob = self._ctx.get_assignments()
        names = np.asarray(self.columns + [None], dtype=object)  # -1 (no non-NaN posterior in the row) -> None
        return pd.DataFrame({'option': names[best], 'probability': prob}, index=self._index())

    def top_options(self, k=2) -> pd.DataFrame:
        """The k <= 4 best options per barcode, best first: columns option_1, probability_1, option_2, ..."""
        options, probs = self._ctx.get_top_options(k)
        names = np.asarray(self.columns + [None], dtype=object)  # -1 (row shorter than k) -> None
        data = {}
        for j in range(options.shape[1]):
            data[f'option_{j + 1}'] = names[options[:, j]]
            data[f'probability_{j + 1}'] = probs[:, j]
        return pd.DataFrame(data, index=self._index())

    def option_sums(self) -> pd.Series:
        """probs.sum(axis=0) (`probs[genotype_names].sum()`, same notebook cells 19 / 21), float64."""
        return pd.Series(self._ctx.get_option_sums(), index=self.columns)

    # ---- donor level: the pair columns of a doublet run folded back onto donors (donor_readout.py) ----
    @property
    def donor_names(self):
        return self.columns[:self.n_donors]

    def doublet_probability(self) -> pd.Series:
        """Per barcode the posterior mass of the pair columns, float64 (0 for a run without doublets):
        probs[pair columns].sum(axis=1) of the DataFrame, added in float64."""
        return pd.Series(self._ctx.get_donor_readout()['doublet_mass'], index=self._index())

    def donor_marginals(self) -> pd.DataFrame:
        """float32 [B, G]: per barcode and donor the posterior mass of every option that contains the donor - its singlet and
        its G - 1 pairs, added in float64 in ascending column order and rounded once.  Without doublets: the posteriors."""
        return pd.DataFrame(self._ctx.get_donor_readout(marginals=True)['donor_marginals'], index=self._index(),
                            columns=self.donor_names)

    def droplet_calls(self, threshold=0.9) -> pd.DataFrame:
        """Per barcode: status, donor_1, donor_2, probability, doublet_probability.
        'singlet' when the best singlet posterior is > threshold (the strict float32 comparison of assignments()): donor_1 is
        that donor, probability its posterior.  Otherwise 'doublet' when the mass of all pair columns is > threshold (float64):
        donor_1, donor_2 are the donors of the most probable pair, probability is that mass.  Otherwise 'unassigned': no donors,
        probability the larger of the two."""
        r = self._ctx.get_donor_readout()
        return donor_readout.compose_calls(self.donor_names, threshold, r['best_singlet'], r['best_singlet_prob'], r['best_pair'],
                                           r['doublet_mass'], index=self._index())

    def donor_summary(self, threshold=0.9) -> pd.DataFrame:
        """Per donor: n_singlets, n_doublets (droplets droplet_calls(threshold) calls doublet whose best pair contains the
        donor) and expected_cells, the float64 column sum of donor_marginals() - formed from option_sums(), a donor's own
        column plus its pair columns, so that nothing of size [B, G] is downloaded."""
        return donor_readout.compose_summary(self.donor_names, self.droplet_calls(threshold), self._ctx.get_option_sums())

    def qualities(self, barcode2possible_options) -> dict:
        """{'logloss', 'accuracy', 'error rate'} of the reference's utils._compute_qualities (utils.py:265-296) against the
        options (column names, pairs as 'A+B') that are possible for each barcode: logloss is the mean of
        -log(max(mass, 1e-4)) with mass the posterior of the barcode's possible options, accuracy the share of barcodes whose
        most probable option is possible.  A barcode that is missing from the dict and a name that is not a column raise
        ValueError (the reference asserts).
        Differs from the reference in precision only: the reference adds the float32 posteriors in float32 and takes a float32
        log; here the masses are float64 sums in list order, formed on the device, and log and mean are float64.  The
        reference's check that the rows sum to one is not repeated."""
        start, options = donor_readout.allowed_lists(self.barcodes, self.columns, barcode2possible_options)
        return donor_readout.compose_qualities(*self._ctx.get_allowed_mass(start, options))

    def rows(self, lo, hi, what='probs') -> pd.DataFrame:
        """Rows [lo, hi) of the 'probs' or 'logits' matrix as a DataFrame."""
        block = self._ctx.get_block(what, lo, hi)
        return pd.DataFrame(block, index=self._index(self.barcodes[lo:hi]), columns=self.columns)

    def to_dataframes(self):
        """(logits_df, probs_df) as the host-side entry points return them."""
        index = self._index()
        return (pd.DataFrame(self._ctx.get_logits(), index=index, columns=self.columns),
                pd.DataFrame(self._ctx.get_probs(), index=index.copy(), columns=self.columns))

    def close(self):
        if self._ctx is not None:
            if self._pooled:
                release_private_context(self._ctx)
            else:
                self._ctx.close()
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Demultiplexer:
    """
    Demultiplexer that can infer (learn) additional information about genotypes to achieve better quality.
    GPU-backed; see the module docstring for what runs where.
    """
    # same knobs as the reference class (demux.py:30-32)
    contribution_power = 2.
    aggregate_on_snps = False
    compensation_during_computing_barcode_logits = 0.5

    # ------------------------------------------------------------------------------------
    @staticmethod
    def learn_genotypes(chromosome2compressed_snp_calls,
                        genotypes,
                        barcode_handler,
                        n_iterations=5,
                        p_genotype_clip=0.01,
                        doublet_prior=0.,
                        barcode_prior_logits: np.ndarray = None,
                        on_device: bool = False,
                        ) -> Tuple[object, pd.DataFrame]:
        """
        Learn genotypes starting from an initial guess (demux.py:35-66).
        :return: learnt genotypes (a copy of `genotypes` with betas = raw betas + the addition used by the
            last E-step) and the barcode-to-donor posteriors of the last iteration.
        The whole loop runs on the GPU (dmx_em); only the last iteration's results come back.
        :param on_device: (not in the reference) leave the posteriors on the GPU and return a DevicePosteriors
            in place of the DataFrame.
        """
        assert 0 <= doublet_prior < 1
        n_genotypes = genotypes.n_genotypes
        penalties = Demultiplexer._doublet_penalties(n_genotypes, doublet_prior)
        if barcode_prior_logits is not None:
            assert barcode_prior_logits.shape == (barcode_handler.n_barcodes, len(penalties)), 'wrong shape of priors'
        assert n_iterations >= 1, 'n_iterations should be positive'  # the reference fails to unpack an empty run

        column_names = _option_names(genotypes.genotype_names, doublet_prior)
        if Demultiplexer.aggregate_on_snps:  # the staged loop is the implementation (float64 posteriors, no fused driver)
            assert not on_device, 'on_device results are float32; aggregate_on_snps yields float64 posteriors'
            *_, (probs_df, last) = Demultiplexer.staged_genotype_learning(
                chromosome2compressed_snp_calls, genotypes, barcode_handler, n_iterations=n_iterations,
                p_genotype_clip=p_genotype_clip, doublet_prior=doublet_prior, barcode_prior_logits=barcode_prior_logits)
            return genotypes._with_betas(genotypes.get_betas() + last['genotype_addition']), probs_df
        if on_device:
            with _handed_over_context() as ctx:
                _pack_on_device(chromosome2compressed_snp_calls, genotypes, barcode_handler.n_barcodes, True,
                                fetch_betas=False, ctx=ctx)
                ctx.em(n_iterations, p_genotype_clip, penalties, with_doublets=doublet_prior != 0,
                       prior_logits=barcode_prior_logits, contribution_power=Demultiplexer.contribution_power,
                       fetch_logits=False, fetch_probs=False, fetch_addition=False)
                learnt_betas = ctx.get_learnt_betas()  # genotypes.get_betas() + addition (demux.py:65), added on the device
            learnt_genotypes = genotypes._with_betas(learnt_betas, _take=True)
            return learnt_genotypes, DevicePosteriors(ctx, barcode_handler.ordered_barcodes, column_names, n_donors=n_genotypes)
        with shared_context_lock:
            ctx, _betas = _pack_on_device(chromosome2compressed_snp_calls, genotypes, barcode_handler.n_barcodes, True,
                                          fetch_betas=False)
            # only the last iteration's posteriors go back to the caller (demux.py:65-66): nobody reads its logits
            ctx.set_logits_needed(False)
            try:
                _logits, probs, _addition = ctx.em(
                    n_iterations, p_genotype_clip, penalties, with_doublets=doublet_prior != 0,
                    prior_logits=barcode_prior_logits, contribution_power=Demultiplexer.contribution_power,
                    fetch_logits=False, fetch_addition=False)
                learnt_betas = ctx.get_learnt_betas()  # genotypes.get_betas() + addition (demux.py:65), added on the device
            finally:
                ctx.set_logits_needed(True)
        probs_df = pd.DataFrame(data=probs, index=_barcode_index(barcode_handler), columns=column_names)
        learnt_genotypes = genotypes._with_betas(learnt_betas, _take=True)
        return learnt_genotypes, probs_df

    @staticmethod
    def staged_genotype_learning(chromosome2compressed_snp_calls,
                                 genotypes,
                                 barcode_handler,
                                 n_iterations=5,
                                 p_genotype_clip=0.01,
                                 doublet_prior=0.,
                                 barcode_prior_logits: np.ndarray = None):
        """Generator over EM iterations (demux.py:69-118): yields (posterior DataFrame, debug dict with
        'barcode_logits', 'genotype_prior', 'genotype_addition'), aligned as in the reference: the yielded
        addition is the one the iteration's E-step used.
        The EM state lives on the GPU between yields, in a device context private to this generator: like the
        reference's (pure) generator it is unaffected by other Demultiplexer calls made between iterations."""
        assert 0 <= doublet_prior < 1
        n_genotypes = genotypes.n_genotypes
        penalties = Demultiplexer._doublet_penalties(n_genotypes, doublet_prior)
        if barcode_prior_logits is not None:
            assert barcode_prior_logits.shape == (barcode_handler.n_barcodes, len(penalties)), 'wrong shape of priors'
        aggregate = bool(Demultiplexer.aggregate_on_snps)  # read once, like the other class-level knobs of a run

        with _generator_context() as ctx:
            ctx.set_keep_molecule_calls(aggregate)
            _ctx, prior_betas = _pack_on_device(chromosome2compressed_snp_calls, genotypes, barcode_handler.n_barcodes,
                                                True, ctx=ctx)
            column_names = _option_names(genotypes.genotype_names, doublet_prior)
            genotype_addition = np.zeros_like(prior_betas)
            ctx.set_addition(None)

            for iteration in range(n_iterations):
                ctx.probs_from_betas(p_genotype_clip, fetch=False)
                prior = barcode_prior_logits if iteration == 0 else None
                if aggregate:  # demux.py:204-244: float64 logits / posteriors, float64 M-step
                    logits, probs = ctx.estep_snp(doublet_prior != 0, Demultiplexer.compensation_during_computing_barcode_logits,
                                                  prior_logits=prior)
                    probs_df = pd.DataFrame(data=probs, index=barcode_handler.ordered_barcodes, columns=column_names)
                    yield probs_df, {
                        'barcode_logits': logits,
                        'genotype_prior': prior_betas,
                        'genotype_addition': genotype_addition,
                    }
                    genotype_addition = ctx.mstep_f64(Demultiplexer.contribution_power)
                    continue
                logits, probs = ctx.estep(penalties, with_doublets=doublet_prior != 0, prior_logits=prior)
                probs_df = pd.DataFrame(data=probs, index=barcode_handler.ordered_barcodes, columns=column_names)
                yield probs_df, {
                    'barcode_logits': logits,
                    'genotype_prior': prior_betas,
                    'genotype_addition': genotype_addition,
                }
                genotype_addition = ctx.mstep(Demultiplexer.contribution_power)

    @staticmethod
    def predict_posteriors(chromosome2compressed_snp_calls,
                           genotypes,
                           barcode_handler,
                           p_genotype_clip=0.01,
                           doublet_prior=0.35,
                           on_device: bool = False):
        """One P + E pass (demux.py:120-156). Returns (logits_df, probs_df), rows in
        barcode_handler.ordered_barcodes order, index named 'BARCODE'.
        :param on_device: (not in the reference) keep logits and posteriors on the GPU and return ONE
            DevicePosteriors object (assignments / top options / column sums are then computed there)."""
        penalties = Demultiplexer._doublet_penalties(genotypes.n_genotypes, doublet_prior)
        column_names = _option_names(genotypes.genotype_names, doublet_prior)
        aggregate = bool(Demultiplexer.aggregate_on_snps)
        assert not (aggregate and on_device), 'on_device results are float32; aggregate_on_snps yields float64 posteriors'

        def run(ctx, fetch):
            ctx.set_keep_molecule_calls(aggregate)  # (read by the pack alone)
            try:
                _set_up_table(ctx, chromosome2compressed_snp_calls, genotypes, barcode_handler.n_barcodes, p_genotype_clip)
            finally:
                ctx.set_keep_molecule_calls(False)
            if aggregate:  # demux.py:204-244
                return ctx.estep_snp(doublet_prior != 0, Demultiplexer.compensation_during_computing_barcode_logits)
            return ctx.estep(penalties, with_doublets=doublet_prior != 0, fetch_logits=fetch, fetch_probs=fetch)

        if on_device:
            with _handed_over_context() as ctx:
                run(ctx, False)
            return DevicePosteriors(ctx, barcode_handler.ordered_barcodes, column_names, index_name='BARCODE',
                                    n_donors=genotypes.n_genotypes)
        with shared_context_lock:
            logits, probs = run(get_context(), True)

        logits_df = pd.DataFrame(data=logits, index=_barcode_index(barcode_handler, 'BARCODE'), columns=column_names)
        probs_df = pd.DataFrame(data=probs, index=_barcode_index(barcode_handler, 'BARCODE'), columns=column_names)  # own Index object, shared labels
        return logits_df, probs_df

    @staticmethod
    def predict_posteriors_in_pools(chromosome2compressed_snp_calls,
                                    genotypes,
                                    barcode_handler,
                                    barcode2pool,
                                    pool2donors,
                                    p_genotype_clip=0.01,
                                    doublet_prior=0.35,
                                    on_device: bool = False) -> PooledPosteriors:
        """(not in the reference) predict_posteriors with every barcode scored against the donors of its own pool only - a
        lane, hashtag group or sub-experiment that holds a known subset of the donors -, all pools in one pass over one packed
        problem and one genotype table.  The frames of a pool (PooledPosteriors.to_dataframes) are, bit for bit, the rows of the
        pool's barcodes in what the reference's predict_posteriors returns for the pool's genotype sub-list on the same table.
        :param barcode2pool: barcode -> pool name, or None for "in no pool"; every barcode of the handler has an entry
        :param pool2donors: pool name -> donor names, in any order (sorted into genotype order); at most 44 donors per pool
            with doublets, 1024 without
        :param on_device: keep the compact logits and posteriors on the GPU and return a DevicePooledPosteriors (best options,
            droplet calls, donor marginals and summaries, option sums and qualities are then computed there)
        ValueError: a duplicate or unknown donor, an empty pool, a barcode without an entry, an unknown pool."""
        assert not Demultiplexer.aggregate_on_snps, 'pooled posteriors are float32; aggregate_on_snps yields float64 posteriors'
        assert 0 <= doublet_prior < 1
        setup = _pool_setup(genotypes, barcode_handler, doublet_prior, barcode2pool, pool2donors, None)

        def run(ctx, fetch=True):
            _set_up_table(ctx, chromosome2compressed_snp_calls, genotypes, barcode_handler.n_barcodes, p_genotype_clip)
            return ctx.estep_pools(setup.pool_columns, setup.pool_of_barcode, doublet_prior != 0, setup.pair_penalty, fetch_logits=fetch,
                                   fetch_probs=fetch)

        if on_device:
            return _pooled_on_device(lambda ctx: run(ctx, False), barcode_handler, setup)[1]
        with shared_context_lock:
            out = run(get_context())
        return _framed_posteriors(setup, barcode_handler, out, 'BARCODE')

    @staticmethod
    def estimate_ambient(chromosome2compressed_snp_calls,
                         genotypes,
                         barcode_handler,
                         assignments,
                         alphas=None,
                         p_genotype_clip=0.01,
                         ambient=None,
                         keep_profile=False) -> AmbientEstimate:
        """(not in the reference) Per-barcode ambient RNA fractions: how much of a droplet's signal is not from the option it was
        assigned to.  For every assigned barcode and every alpha of the grid, the log-likelihood of its calls when a share alpha of
        its molecules comes from the soup (allele profile `ambient`) and the rest from its donor(s); the estimate is the grid value
        of the first maximum (AmbientEstimate.summary()).  At alpha = 0 the likelihood of a singlet is, bit for bit, the donor's
        column of predict_posteriors' logits.
        :param assignments: Series or mapping barcode -> option name (as predict_posteriors' columns or DevicePosteriors.best()
            give it; looked up exactly, so donor names may contain '+'), integer option column, or None / NaN / -1 to skip; a
            barcode that is not mentioned is skipped
        :param alphas: the grid, 1 .. 64 values in [0, 1] in any order; None: 0, 0.01 .. 0.63
        :param ambient: float32[n_variants] allele profile of the soup per variant row, or None: derived from the calls (per SNP
            the share of every allele among the barcode-level calls, one pseudo-count each, clipped like the genotype table)
        :param keep_profile: also return the [B, A] log-likelihoods (AmbientEstimate.profile)
        ValueError: an unknown option name, a column outside the options, a barcode that is not the handler's."""
        assert not Demultiplexer.aggregate_on_snps, 'ambient fractions are estimated on barcode-level calls; aggregate_on_snps has none'
        names = list(genotypes.genotype_names)
        option_names = _option_names(names, 1)  # every option a run with doublets can assign; a singlet run's names are its first G
        columns = resolve_assignments(option_names, barcode_handler.ordered_barcodes, assignments)
        donor1, donor2 = assigned_donors(len(names), columns)
        alphas = default_alphas() if alphas is None else np.ascontiguousarray(alphas, dtype=np.float32).reshape(-1)
        with shared_context_lock:
            ctx = get_context()
            _set_up_table(ctx, chromosome2compressed_snp_calls, genotypes, barcode_handler.n_barcodes, p_genotype_clip)
            out = ctx.ambient_profile(donor1, donor2, alphas, p_genotype_clip, ambient=ambient, fetch_profile=keep_profile)
        return AmbientEstimate(barcode_handler.ordered_barcodes, option_names, columns, alphas, out['ambient'], out['best'], out['ll_best'],
                               out['ll_zero'], loglik=out['loglik'], index_name='BARCODE')

    @staticmethod
    def _ambient_setup(genotypes, barcode_handler, ambient_fractions, doublet_prior, barcode2pool, pool2donors, who):
        """What the entries under per-barcode ambient fractions refuse and resolve, in this order: (alpha float32[B], the _PoolSetup)."""
        assert not Demultiplexer.aggregate_on_snps, 'ambient fractions act on barcode-level calls; aggregate_on_snps has none'
        assert 0 <= doublet_prior < 1
        assert (barcode2pool is None) == (pool2donors is None), 'barcode2pool and pool2donors come together'
        alpha = resolve_fractions(barcode_handler.ordered_barcodes, ambient_fractions)
        return alpha, _pool_setup(genotypes, barcode_handler, doublet_prior, barcode2pool, pool2donors, who)

    @staticmethod
    def predict_posteriors_with_ambient(chromosome2compressed_snp_calls,
                                        genotypes,
                                        barcode_handler,
                                        ambient_fractions,
                                        ambient=None,
                                        p_genotype_clip=0.01,
                                        doublet_prior=0.35,
                                        barcode2pool=None,
                                        pool2donors=None,
                                        on_device: bool = False):
        """(not in the reference) predict_posteriors with every option scored under the barcode's own ambient fraction: a call's
        term is q (1 - alpha_b) + ambient[v] alpha_b in place of the option's q, so a contaminated singlet - its donor plus a little
        of everybody - is not taken for a doublet.  With every fraction 0 the result is predict_posteriors' (exact mode) bit for bit.
        :param ambient_fractions: Series or mapping barcode -> alpha in [0, 1] (AmbientEstimate.fractions() gives one); a barcode
            that is missing, None or NaN is scored with 0
        :param ambient: float32[n_variants] allele profile of the soup, or None: derived from the calls as estimate_ambient does
        :param barcode2pool, pool2donors: as predict_posteriors_in_pools takes them (both or neither)
        :param on_device: keep the compact rows on the GPU and return a DevicePooledPosteriors (without pools it holds the one
            all-donor pool, named 'all')
        Returns (logits_df, probs_df) with predict_posteriors' index, columns and dtypes; with pools a PooledPosteriors.
        ValueError: a fraction outside [0, 1], a barcode that is not the handler's, more than 1024 options without pools."""
        alpha, setup = Demultiplexer._ambient_setup(genotypes, barcode_handler, ambient_fractions, doublet_prior, barcode2pool, pool2donors,
                                                    'predict_posteriors_with_ambient')

        def run(ctx, fetch=True):
            _set_up_table(ctx, chromosome2compressed_snp_calls, genotypes, barcode_handler.n_barcodes, p_genotype_clip)
            return ctx.estep_ambient(setup.pool_columns, setup.pool_of_barcode, doublet_prior != 0, setup.pair_penalty, alpha, p_genotype_clip,
                                     ambient=ambient, fetch_logits=fetch, fetch_probs=fetch)

        if on_device:
            return _pooled_on_device(lambda ctx: run(ctx, False), barcode_handler, setup)[1]
        with shared_context_lock:
            out = run(get_context())
        return _framed_posteriors(setup, barcode_handler, out, 'BARCODE')

    @staticmethod
    def predict_posteriors_decontaminated(chromosome2compressed_snp_calls,
                                          genotypes,
                                          barcode_handler,
                                          alphas=None,
                                          ambient=None,
                                          p_genotype_clip=0.01,
                                          doublet_prior=0.35):
        """(not in the reference) Three passes over one packed, resident problem: (1) plain posteriors, in the exact arithmetic;
        (2) estimate_ambient with every barcode assigned its best SINGLET - the first maximum over the singlet columns of the plain
        logits (their penalty is 0: the donors' log-likelihoods), whatever the doublet columns say, since a contaminated singlet is
        exactly what the plain pass takes for a doublet; (3) predict_posteriors_with_ambient with those fractions and the same soup
        profile.  Returns (logits_df, probs_df, AmbientEstimate): the re-scored frames and the estimate of pass 2.
        The fractions are estimated under the singlet hypothesis: part of a true doublet's second donor can be absorbed as
        contamination.
        :param alphas, ambient: as estimate_ambient takes them
        ValueError: more than 1024 options (44 donors with doublets)."""
        assert not Demultiplexer.aggregate_on_snps, 'ambient fractions act on barcode-level calls; aggregate_on_snps has none'
        assert 0 <= doublet_prior < 1
        names = list(genotypes.genotype_names)
        G = len(names)
        setup = _pool_setup(genotypes, barcode_handler, doublet_prior, None, None, 'predict_posteriors_decontaminated')
        alphas = default_alphas() if alphas is None else np.ascontiguousarray(alphas, dtype=np.float32).reshape(-1)
        B, with_doublets = barcode_handler.n_barcodes, doublet_prior != 0
        with shared_context_lock:
            ctx = get_context()
            _set_up_table(ctx, chromosome2compressed_snp_calls, genotypes, B, p_genotype_clip)
            plain = ctx.estep_pools(setup.pool_columns, setup.pool_of_barcode, with_doublets, setup.pair_penalty, fetch_probs=False)
            columns = best_singlets(plain['logits'].reshape(B, len(setup.option_names[0])), G)
            donor1, donor2 = assigned_donors(G, columns)
            profile = ctx.ambient_profile(donor1, donor2, alphas, p_genotype_clip, ambient=ambient, fetch_profile=False)
            estimate = AmbientEstimate(barcode_handler.ordered_barcodes, _option_names(names, 1), columns, alphas, profile['ambient'],
                                       profile['best'], profile['ll_best'], profile['ll_zero'], index_name='BARCODE')
            alpha = np.nan_to_num(estimate.fractions().values, nan=0.0).astype(np.float32)
            out = ctx.estep_ambient(setup.pool_columns, setup.pool_of_barcode, with_doublets, setup.pair_penalty, alpha, p_genotype_clip,
                                    ambient=profile['ambient'])
        return (*_framed_posteriors(setup, barcode_handler, out, 'BARCODE'), estimate)

    @staticmethod
    def predict_posteriors_joint_ambient(chromosome2compressed_snp_calls,
                                         genotypes,
                                         barcode_handler,
                                         alphas=None,
                                         ambient=None,
                                         p_genotype_clip=0.01,
                                         doublet_prior=0.35,
                                         barcode2pool=None,
                                         pool2donors=None,
                                         keep_profile=False,
                                         over_grid='max',
                                         alpha_log_weights=None,
                                         on_device: bool = False) -> JointAmbientPosteriors:
        """(not in the reference) predict_posteriors with every option - singlets and pairs - scored at its own best ambient
        fraction: a call's term is q (1 - alpha) + ambient[v] alpha, an option's logit the maximum over the grid `alphas` of its
        log-likelihood (plus the pair penalty), and the posteriors one softmax over those.  The choice between "a contaminated
        singlet" and "a doublet" is made inside that softmax, in one pass, where predict_posteriors_decontaminated estimates the
        fraction under the best singlet first and so explains a true doublet's second donor as contamination.
        With alphas=[0.0] the result is predict_posteriors' (exact mode) bit for bit.
        :param alphas: the grid, 1 .. 64 values in [0, 1] in any order; None: 0, 0.01 .. 0.63
        :param ambient: float32[n_variants] allele profile of the soup, or None: derived from the calls as estimate_ambient does
        :param barcode2pool, pool2donors: as predict_posteriors_in_pools takes them (both or neither)
        :param keep_profile: also return every option's logit at every grid point (JointAmbientPosteriors.profile: the grid's
            length times the logits' memory)
        :param over_grid: 'max' (the default, as above) or 'marginal': an option's logit is the log of the sum over the grid of
            exp(log-likelihood + alpha_log_weights) - an option that fits over a wide range of fractions is credited for it, which
            finds more of the true doublets among droplets with few calls.  With alphas=[0.0] both are
            predict_posteriors'.  'marginal' keeps no profile: with keep_profile it raises.
        :param alpha_log_weights: ('marginal' only) the log of a prior over the grid, one finite value per grid value; None: flat
        :param on_device: keep the compact rows - logits, posteriors, every option's grid point and mean fraction - on the GPU and
            return a DeviceJointAmbientPosteriors, whose .posteriors is a DevicePooledPosteriors (without pools: one pool, 'all');
            with keep_profile it raises
        Returns a JointAmbientPosteriors: .posteriors is (logits_df, probs_df) with predict_posteriors' index, columns and dtypes,
        with pools a PooledPosteriors; .option_alphas, .summary(); under 'marginal' also .option_alpha_means.
        ValueError: a grid value outside [0, 1], an empty grid or more than 64 values, more than 1024 options without pools,
        over_grid='marginal' with keep_profile, alpha_log_weights with over_grid='max'."""
        if over_grid not in ('max', 'marginal'):
            raise ValueError(f"over_grid is 'max' or 'marginal', not {over_grid!r}")
        if over_grid == 'marginal' and keep_profile:
            raise ValueError("keep_profile needs over_grid='max': the marginal pass keeps no profile")
        if alpha_log_weights is not None and over_grid != 'marginal':
            raise ValueError("alpha_log_weights are the prior of over_grid='marginal'; the maximum takes none")
        if on_device and keep_profile:
            raise ValueError('keep_profile with on_device: the profile is not kept on the device; ask for it with on_device=False')
        assert not Demultiplexer.aggregate_on_snps, 'ambient fractions act on barcode-level calls; aggregate_on_snps has none'
        assert 0 <= doublet_prior < 1
        assert (barcode2pool is None) == (pool2donors is None), 'barcode2pool and pool2donors come together'
        grid = resolve_grid(alphas)
        if alpha_log_weights is not None:
            alpha_log_weights = np.ascontiguousarray(alpha_log_weights, dtype=np.float32).reshape(-1)
            if alpha_log_weights.shape != grid.shape or not np.isfinite(alpha_log_weights).all():
                raise ValueError('alpha_log_weights: one finite value per grid value')
        setup = _pool_setup(genotypes, barcode_handler, doublet_prior, barcode2pool, pool2donors, 'predict_posteriors_joint_ambient')

        def run(ctx, fetch=True):
            _set_up_table(ctx, chromosome2compressed_snp_calls, genotypes, barcode_handler.n_barcodes, p_genotype_clip)
            pools = (setup.pool_columns, setup.pool_of_barcode, doublet_prior != 0, setup.pair_penalty)
            if over_grid == 'marginal':
                return ctx.estep_ambient_grid(*pools, grid, p_genotype_clip, ambient=ambient, over_grid='marginal', log_weights=alpha_log_weights,
                                              fetch_logits=fetch, fetch_probs=fetch, fetch_alpha_index=fetch, fetch_alpha_mean=fetch)
            return ctx.estep_ambient_grid(*pools, grid, p_genotype_clip, ambient=ambient, fetch_profile=keep_profile, fetch_logits=fetch,
                                          fetch_probs=fetch, fetch_alpha_index=fetch)

        if on_device:
            out, posteriors = _pooled_on_device(lambda ctx: run(ctx, False), barcode_handler, setup)
            return DeviceJointAmbientPosteriors(posteriors, grid, out['ambient'], out['best_alpha_index'], over_grid=over_grid,
                                                best_alpha_mean=out.get('best_alpha_mean'))
        with shared_context_lock:
            out = run(get_context())
        return JointAmbientPosteriors(barcode_handler.ordered_barcodes, setup.option_names, setup.pool_of_barcode, out['row_ptr'], grid, out['ambient'],
                                      out['alpha_index'], out['best_option'], out['best_prob'], out['doublet_mass'], out['best_alpha_index'],
                                      _framed_posteriors(setup, barcode_handler, out, 'BARCODE'), profile=out['profile'], index_name='BARCODE', over_grid=over_grid,
                                      alpha_mean=out.get('alpha_mean'), best_alpha_mean=out.get('best_alpha_mean'))

    @staticmethod
    def predict_posteriors_with_doublet_shares(chromosome2compressed_snp_calls,
                                               genotypes,
                                               barcode_handler,
                                               shares=None,
                                               share_log_weights=None,
                                               p_genotype_clip=0.01,
                                               doublet_prior=0.35,
                                               barcode2pool=None,
                                               pool2donors=None) -> DoubletSharePosteriors:
        """(not in the reference) predict_posteriors / predict_posteriors_in_pools with every pair option scored as the marginal over
        a grid of mixing shares: a call's term for the pair 'A+B' is prob[A] w + prob[B] (1 - w) in place of the even
        (prob[A] + prob[B]) / 2, the pair's logit the log of the sum over the grid of exp(log-likelihood + share_log_weights) plus the
        pair penalty.  Two cells of different RNA content share a droplet unevenly, and an 80 / 20 doublet scored at 0.5 looks like
        its major donor.  Singlet options are predict_posteriors'.  One pass over the resident problem.
        With shares=[0.5] and share_log_weights=[0.0] the result is predict_posteriors' (exact mode) bit for bit.
        :param shares: the grid of shares of the first-named donor, 1 .. 64 values in [0, 1] in any order; None: 0.1, 0.2 .. 0.9
        :param share_log_weights: the log of a prior over the grid, one finite value per share; None: uniform, -log(n) each.  The
            normalisation matters: singlets do not go through the grid
        :param barcode2pool, pool2donors: as predict_posteriors_in_pools takes them (both or neither)
        Returns a DoubletSharePosteriors: .posteriors is (logits_df, probs_df) with predict_posteriors' index, columns and dtypes,
        with pools a PooledPosteriors; .option_shares, .option_share_index, .summary().
        ValueError: a share outside [0, 1], an empty grid or more than 64 values, weights that do not fit the grid, more than 1024
        options without pools (give pools with barcode2pool / pool2donors)."""
        assert not Demultiplexer.aggregate_on_snps, 'doublet shares act on barcode-level calls; aggregate_on_snps has none'
        assert 0 <= doublet_prior < 1
        assert (barcode2pool is None) == (pool2donors is None), 'barcode2pool and pool2donors come together'
        grid, log_weights = resolve_shares(shares, share_log_weights)
        setup = _pool_setup(genotypes, barcode_handler, doublet_prior, barcode2pool, pool2donors, 'predict_posteriors_with_doublet_shares')
        with shared_context_lock:
            ctx = get_context()
            _set_up_table(ctx, chromosome2compressed_snp_calls, genotypes, barcode_handler.n_barcodes, p_genotype_clip)
            out = ctx.estep_pair_shares(setup.pool_columns, setup.pool_of_barcode, doublet_prior != 0, setup.pair_penalty, grid, log_weights)
        names = list(genotypes.genotype_names)
        return DoubletSharePosteriors(barcode_handler.ordered_barcodes, setup.option_names, [[names[g] for g in columns] for columns in setup.pool_columns],
                                      setup.pool_of_barcode, out['row_ptr'], grid, log_weights, out['share_index'], out['share_mean'],
                                      out['best_option'], out['best_prob'], out['doublet_mass'], out['best_share_index'], out['best_share_mean'],
                                      _framed_posteriors(setup, barcode_handler, out, 'BARCODE'), index_name='BARCODE')

    @staticmethod
    def learn_genotypes_in_pools(chromosome2compressed_snp_calls,
                                 genotypes,
                                 barcode_handler,
                                 barcode2pool,
                                 pool2donors,
                                 n_iterations=5,
                                 p_genotype_clip=0.01,
                                 doublet_prior=0.) -> Tuple[object, PooledPosteriors]:
        """(not in the reference) learn_genotypes with every barcode scored against the donors of its own pool only: the
        reference's loop (demux.py:86-118) with the E-step of predict_posteriors_in_pools, and posterior 0 for the donors outside
        a barcode's pool.  A barcode in no pool contributes nothing; a donor in no pool keeps its betas.  With one all-donor pool
        this is learn_genotypes itself.  The whole loop runs on the GPU (dmx_em_pools).
        :param barcode2pool, pool2donors: as in predict_posteriors_in_pools (same ValueErrors)
        :return: learnt genotypes (betas = raw betas + the addition used by the last E-step) and the PooledPosteriors of the
            last iteration."""
        assert not Demultiplexer.aggregate_on_snps, 'pooled posteriors are float32; aggregate_on_snps yields float64 posteriors'
        assert 0 <= doublet_prior < 1
        assert n_iterations >= 1, 'n_iterations should be positive'
        setup = _pool_setup(genotypes, barcode_handler, doublet_prior, barcode2pool, pool2donors, None)
        with shared_context_lock:
            ctx, _betas = _pack_on_device(chromosome2compressed_snp_calls, genotypes, barcode_handler.n_barcodes, True,
                                          fetch_betas=False)
            out = ctx.em_pools(n_iterations, p_genotype_clip, setup.pool_columns, setup.pool_of_barcode, doublet_prior != 0, setup.pair_penalty,
                               contribution_power=Demultiplexer.contribution_power, fetch_addition=False)
            learnt_betas = ctx.get_learnt_betas()  # genotypes.get_betas() + addition (demux.py:65), added on the device
        return genotypes._with_betas(learnt_betas, _take=True), _framed_posteriors(setup, barcode_handler, out, None)

    @staticmethod
    def staged_genotype_learning_in_pools(chromosome2compressed_snp_calls,
                                          genotypes,
                                          barcode_handler,
                                          barcode2pool,
                                          pool2donors,
                                          n_iterations=5,
                                          p_genotype_clip=0.01,
                                          doublet_prior=0.):
        """Generator over the iterations of learn_genotypes_in_pools, shaped like staged_genotype_learning: yields
        (PooledPosteriors, debug dict with 'genotype_prior', 'genotype_addition'); the yielded addition is the one the
        iteration's E-step used.  The EM state lives on the GPU between yields, in a device context private to this generator."""
        assert not Demultiplexer.aggregate_on_snps, 'pooled posteriors are float32; aggregate_on_snps yields float64 posteriors'
        assert 0 <= doublet_prior < 1
        setup = _pool_setup(genotypes, barcode_handler, doublet_prior, barcode2pool, pool2donors, None)

        with _generator_context() as ctx:
            _ctx, prior_betas = _pack_on_device(chromosome2compressed_snp_calls, genotypes, barcode_handler.n_barcodes, True, ctx=ctx)
            genotype_addition = np.zeros_like(prior_betas)
            ctx.set_addition(None)
            for _iteration in range(n_iterations):
                ctx.probs_from_betas(p_genotype_clip, fetch=False)
                out = ctx.estep_pools(setup.pool_columns, setup.pool_of_barcode, doublet_prior != 0, setup.pair_penalty, resident=True)
                yield _framed_posteriors(setup, barcode_handler, out, None), {
                    'genotype_prior': prior_betas,
                    'genotype_addition': genotype_addition,
                }
                genotype_addition = ctx.mstep(Demultiplexer.contribution_power)

    @staticmethod
    def learn_genotypes_with_ambient(chromosome2compressed_snp_calls,
                                     genotypes,
                                     barcode_handler,
                                     ambient_fractions,
                                     ambient=None,
                                     n_iterations=5,
                                     p_genotype_clip=0.01,
                                     doublet_prior=0.,
                                     barcode2pool=None,
                                     pool2donors=None):
        """(not in the reference) learn_genotypes for contaminated droplets: the loop of learn_genotypes_in_pools with every option
        scored under the barcode's own ambient fraction (predict_posteriors_with_ambient's E-step) and every call's contribution to
        the betas weighted by the probability that the call came from the donor and not from the soup,
        r = own / (own + ambient[v] alpha_b) with own = genotype_prob[v, g] (1 - alpha_b) - at alpha = 0.4 four calls in ten come from
        the soup and would pull the donor's betas towards the population mean.  With every fraction 0 the result is
        learn_genotypes_in_pools' (exact mode) bit for bit.  The fractions and the soup's profile are fixed for the call (alternate
        estimate_ambient and this call to refine the fractions; learn_genotypes_and_ambient learns the profile along with the genotypes).  The whole loop runs on the GPU (dmx_em_ambient); its sums are float64 in the
        reference's order whatever DEMUXALOT_AMD_ESTEP says.
        :param ambient_fractions: Series or mapping barcode -> alpha in [0, 1] (AmbientEstimate.fractions() gives one); a barcode
            that is missing, None or NaN learns with 0
        :param ambient: float32[n_variants] allele profile of the soup, or None: derived from the calls as estimate_ambient does
        :param barcode2pool, pool2donors: as learn_genotypes_in_pools takes them (both or neither); without them every barcode is
            scored against all donors
        :return: learnt genotypes (betas = raw betas + the addition used by the last E-step) and the posteriors of the last
            iteration: probs_df as learn_genotypes returns it, or with pools a PooledPosteriors.
        ValueError: a fraction outside [0, 1], a barcode that is not the handler's, more than 1024 options without pools."""
        assert n_iterations >= 1, 'n_iterations should be positive'
        alpha, setup = Demultiplexer._ambient_setup(genotypes, barcode_handler, ambient_fractions, doublet_prior, barcode2pool, pool2donors,
                                                    'learn_genotypes_with_ambient')
        with shared_context_lock:
            ctx, _betas = _pack_on_device(chromosome2compressed_snp_calls, genotypes, barcode_handler.n_barcodes, True,
                                          fetch_betas=False)
            out = ctx.em_ambient(n_iterations, p_genotype_clip, setup.pool_columns, setup.pool_of_barcode, doublet_prior != 0, setup.pair_penalty,
                                 alpha, ambient=ambient, contribution_power=Demultiplexer.contribution_power, fetch_logits=setup.pooled,
                                 fetch_addition=False)
            learnt_betas = ctx.get_learnt_betas()  # genotypes.get_betas() + addition (demux.py:65), added on the device
        return genotypes._with_betas(learnt_betas, _take=True), _framed_posteriors(setup, barcode_handler, out, None)

    @staticmethod
    def staged_genotype_learning_with_ambient(chromosome2compressed_snp_calls,
                                              genotypes,
                                              barcode_handler,
                                              ambient_fractions,
                                              ambient=None,
                                              n_iterations=5,
                                              p_genotype_clip=0.01,
                                              doublet_prior=0.,
                                              barcode2pool=None,
                                              pool2donors=None):
        """Generator over the iterations of learn_genotypes_with_ambient, shaped like staged_genotype_learning_in_pools: yields
        (posteriors, debug dict with 'genotype_prior', 'genotype_addition', 'ambient'); the posteriors are a PooledPosteriors with
        pools and probs_df without, the yielded addition is the one the iteration's E-step used, 'ambient' the soup's profile in use
        (the one of the first iteration is kept for the later ones).  The EM state lives on the GPU between yields, in a device
        context private to this generator."""
        alpha, setup = Demultiplexer._ambient_setup(genotypes, barcode_handler, ambient_fractions, doublet_prior, barcode2pool, pool2donors,
                                                    'staged_genotype_learning_with_ambient')

        with _generator_context() as ctx:
            _ctx, prior_betas = _pack_on_device(chromosome2compressed_snp_calls, genotypes, barcode_handler.n_barcodes, True, ctx=ctx)
            genotype_addition = np.zeros_like(prior_betas)
            ctx.set_addition(None)
            for _iteration in range(n_iterations):
                ctx.probs_from_betas(p_genotype_clip, fetch=False)
                out = ctx.estep_ambient(setup.pool_columns, setup.pool_of_barcode, doublet_prior != 0, setup.pair_penalty, alpha, p_genotype_clip,
                                        ambient=ambient, fetch_logits=setup.pooled, resident=True)
                ambient = out['ambient']  # (a derived profile depends on the calls only: the same every iteration)
                yield _framed_posteriors(setup, barcode_handler, out, None), {
                    'genotype_prior': prior_betas,
                    'genotype_addition': genotype_addition,
                    'ambient': ambient,
                }
                genotype_addition = ctx.mstep_ambient(alpha, Demultiplexer.contribution_power, p_genotype_clip, ambient=ambient)

    @staticmethod
    def learn_ambient_profile(chromosome2compressed_snp_calls,
                              genotypes,
                              barcode_handler,
                              ambient_fractions,
                              ambient=None,
                              n_iterations=3,
                              pseudo_count=1.,
                              p_genotype_clip=0.01,
                              doublet_prior=0.,
                              barcode2pool=None,
                              pool2donors=None) -> np.ndarray:
        """(not in the reference) The soup's allele profile learnt from the calls, with the genotypes fixed: n_iterations of
        predict_posteriors_with_ambient's E-step (resident) and the soup M-step behind it - every call counts for the soup with
        the probability that it came from there and not from its donor, s = amb / (own + amb), amb = ambient[v] alpha_b,
        own = genotype_prob[v, g] (1 - alpha_b); per variant the posterior-weighted sum of s gives the soup's expected calls, and
        the new profile is their share within each SNP (one pseudo_count per variant, clipped as the genotype table is).  The derived
        profile (ambient=None: every call of a SNP counted) is the soup only when the soup is the droplets' average; a soup
        dominated by one lysed sample is pulled towards the population mean there, and this call pulls it back.
        :param ambient_fractions: Series or mapping barcode -> alpha in [0, 1] (AmbientEstimate.fractions() gives one); a barcode
            that is missing, None or NaN counts with 0 - and so not at all
        :param ambient: float32[n_variants], the profile to start from, or None: derived from the calls as estimate_ambient does
        :param barcode2pool, pool2donors: as predict_posteriors_in_pools takes them (both or neither)
        :return: float32[n_variants], the profile after the last update.
        ValueError: a fraction outside [0, 1], a barcode that is not the handler's, more than 1024 options without pools."""
        assert n_iterations >= 1, 'n_iterations should be positive'
        assert np.isfinite(pseudo_count) and pseudo_count > 0, 'pseudo_count should be finite and positive'
        alpha, setup = Demultiplexer._ambient_setup(genotypes, barcode_handler, ambient_fractions, doublet_prior, barcode2pool, pool2donors,
                                                    'learn_ambient_profile')
        with shared_context_lock:
            ctx = get_context()
            _set_up_table(ctx, chromosome2compressed_snp_calls, genotypes, barcode_handler.n_barcodes, p_genotype_clip)
            for _iteration in range(n_iterations):
                out = ctx.estep_ambient(setup.pool_columns, setup.pool_of_barcode, doublet_prior != 0, setup.pair_penalty, alpha, p_genotype_clip,
                                        ambient=ambient, fetch_logits=False, fetch_probs=False, resident=True)
                ambient, _counts = ctx.mstep_soup(alpha, pseudo_count, p_genotype_clip, ambient=out['ambient'])
        return ambient

    @staticmethod
    def learn_genotypes_and_ambient(chromosome2compressed_snp_calls,
                                    genotypes,
                                    barcode_handler,
                                    ambient_fractions,
                                    ambient=None,
                                    n_iterations=5,
                                    pseudo_count=1.,
                                    p_genotype_clip=0.01,
                                    doublet_prior=0.,
                                    barcode2pool=None,
                                    pool2donors=None):
        """(not in the reference) learn_genotypes_with_ambient with the soup's profile learnt along with the genotypes: behind every
        E-step but the last, learn_ambient_profile's soup M-step and the weighted genotype M-step, both with the profile that
        E-step read; the new profile takes effect in the next iteration.  The fractions stay fixed (estimate_ambient gives them).
        The whole loop runs on the GPU (dmx_em_ambient_soup).
        :param ambient: float32[n_variants], the first iteration's profile, or None: derived from the calls
        :param pseudo_count: added to every variant's expected soup calls before their share within the SNP is taken
        :return: (learnt genotypes, the posteriors of the last iteration as learn_genotypes_with_ambient returns them, float32
            [n_variants]: the profile the last E-step read).
        ValueError: as learn_genotypes_with_ambient."""
        assert n_iterations >= 1, 'n_iterations should be positive'
        assert np.isfinite(pseudo_count) and pseudo_count > 0, 'pseudo_count should be finite and positive'
        alpha, setup = Demultiplexer._ambient_setup(genotypes, barcode_handler, ambient_fractions, doublet_prior, barcode2pool, pool2donors,
                                                    'learn_genotypes_and_ambient')
        with shared_context_lock:
            ctx, _betas = _pack_on_device(chromosome2compressed_snp_calls, genotypes, barcode_handler.n_barcodes, True,
                                          fetch_betas=False)
            out = ctx.em_ambient_soup(n_iterations, p_genotype_clip, setup.pool_columns, setup.pool_of_barcode, doublet_prior != 0,
                                      setup.pair_penalty, alpha, ambient=ambient, pseudo_count=pseudo_count,
                                      contribution_power=Demultiplexer.contribution_power, fetch_logits=setup.pooled, fetch_addition=False)
            learnt_betas = ctx.get_learnt_betas()  # genotypes.get_betas() + addition (demux.py:65), added on the device
        return genotypes._with_betas(learnt_betas, _take=True), _framed_posteriors(setup, barcode_handler, out, None), out['ambient']

    @staticmethod
    def staged_genotype_learning_and_ambient(chromosome2compressed_snp_calls,
                                             genotypes,
                                             barcode_handler,
                                             ambient_fractions,
                                             ambient=None,
                                             n_iterations=5,
                                             pseudo_count=1.,
                                             p_genotype_clip=0.01,
                                             doublet_prior=0.,
                                             barcode2pool=None,
                                             pool2donors=None):
        """Generator over the iterations of learn_genotypes_and_ambient: yields what staged_genotype_learning_with_ambient yields -
        (posteriors, debug dict with 'genotype_prior', 'genotype_addition', 'ambient') -, 'ambient' the profile that the
        iteration's E-step read.  The EM state lives on the GPU between yields, in a device context private to this generator."""
        assert n_iterations >= 1, 'n_iterations should be positive'
        assert np.isfinite(pseudo_count) and pseudo_count > 0, 'pseudo_count should be finite and positive'
        alpha, setup = Demultiplexer._ambient_setup(genotypes, barcode_handler, ambient_fractions, doublet_prior, barcode2pool, pool2donors,
                                                    'staged_genotype_learning_and_ambient')

        with _generator_context() as ctx:
            _ctx, prior_betas = _pack_on_device(chromosome2compressed_snp_calls, genotypes, barcode_handler.n_barcodes, True, ctx=ctx)
            genotype_addition = np.zeros_like(prior_betas)
            ctx.set_addition(None)
            for _iteration in range(n_iterations):
                ctx.probs_from_betas(p_genotype_clip, fetch=False)
                out = ctx.estep_ambient(setup.pool_columns, setup.pool_of_barcode, doublet_prior != 0, setup.pair_penalty, alpha, p_genotype_clip,
                                        ambient=ambient, fetch_logits=setup.pooled, resident=True)
                read = out['ambient']
                yield _framed_posteriors(setup, barcode_handler, out, None), {
                    'genotype_prior': prior_betas,
                    'genotype_addition': genotype_addition,
                    'ambient': read,
                }
                if _iteration + 1 == n_iterations:
                    break  # (the M-steps after the last yield are dead)
                ambient, _counts = ctx.mstep_soup(alpha, pseudo_count, p_genotype_clip, ambient=read)
                genotype_addition = ctx.mstep_ambient(alpha, Demultiplexer.contribution_power, p_genotype_clip, ambient=read)

    @staticmethod
    def _doublet_learning_setup(genotypes, barcode_handler, doublet_prior, min_pair_posterior, barcode2pool, pool2donors, who):
        """What the entries that learn from doublets refuse and resolve: the _PoolSetup."""
        assert not Demultiplexer.aggregate_on_snps, 'pooled posteriors are float32; aggregate_on_snps yields float64 posteriors'
        assert 0 <= doublet_prior < 1
        assert (barcode2pool is None) == (pool2donors is None), 'barcode2pool and pool2donors come together'
        if not (np.isfinite(min_pair_posterior) and min_pair_posterior > 0):
            raise ValueError(f'{who}: min_pair_posterior must be finite and above 0, not {min_pair_posterior!r}')
        return _pool_setup(genotypes, barcode_handler, doublet_prior, barcode2pool, pool2donors, who)

    @staticmethod
    def learn_genotypes_from_doublets(chromosome2compressed_snp_calls,
                                      genotypes,
                                      barcode_handler,
                                      n_iterations=5,
                                      p_genotype_clip=0.01,
                                      doublet_prior=0.35,
                                      min_pair_posterior=1e-3,
                                      barcode2pool=None,
                                      pool2donors=None):
        """(not in the reference) learn_genotypes that also learns from the droplets it recognises as doublets: the loop of
        learn_genotypes_in_pools whose M-step credits each donor of a pair option 'A+B' with its share of every call of the
        barcode, r = genotype_prob[v, A] / (genotype_prob[v, A] + genotype_prob[v, B]) - the donor's responsibility for the call in
        the even mixture the pair is scored with -, weighted by the pair's posterior.  The reference learns from the singlet
        columns only, so with doublet_prior = 0.35 a third of a loaded lane teaches nothing.  With
        doublet_prior = 0, or min_pair_posterior above 1, the result is learn_genotypes_in_pools' (exact mode) bit for bit.  The
        whole loop runs on the GPU (dmx_em_doublets); its sums are float64 in the reference's order whatever DEMUXALOT_AMD_ESTEP
        says.
        :param min_pair_posterior: a pair option is credited when its posterior is at least this (finite, above 0); the pairs
            left out at the default would have added at most 1e-6 to a weight
        :param barcode2pool, pool2donors: as learn_genotypes_in_pools takes them (both or neither); without them every barcode is
            scored against all donors
        :return: learnt genotypes (betas = raw betas + the addition used by the last E-step) and the posteriors of the last
            iteration: probs_df as learn_genotypes returns it, or with pools a PooledPosteriors.
        ValueError: a threshold that is not finite or not above 0, more than 1024 options without pools."""
        assert n_iterations >= 1, 'n_iterations should be positive'
        setup = Demultiplexer._doublet_learning_setup(genotypes, barcode_handler, doublet_prior, min_pair_posterior, barcode2pool, pool2donors,
                                                      'learn_genotypes_from_doublets')
        with shared_context_lock:
            ctx, _betas = _pack_on_device(chromosome2compressed_snp_calls, genotypes, barcode_handler.n_barcodes, True,
                                          fetch_betas=False)
            out = ctx.em_doublets(n_iterations, p_genotype_clip, setup.pool_columns, setup.pool_of_barcode, doublet_prior != 0, setup.pair_penalty,
                                  min_pair_posterior, contribution_power=Demultiplexer.contribution_power, fetch_logits=setup.pooled,
                                  fetch_addition=False)
            learnt_betas = ctx.get_learnt_betas()  # genotypes.get_betas() + addition (demux.py:65), added on the device
        return genotypes._with_betas(learnt_betas, _take=True), _framed_posteriors(setup, barcode_handler, out, None)

    @staticmethod
    def staged_genotype_learning_from_doublets(chromosome2compressed_snp_calls,
                                               genotypes,
                                               barcode_handler,
                                               n_iterations=5,
                                               p_genotype_clip=0.01,
                                               doublet_prior=0.35,
                                               min_pair_posterior=1e-3,
                                               barcode2pool=None,
                                               pool2donors=None):
        """Generator over the iterations of learn_genotypes_from_doublets, shaped like staged_genotype_learning_in_pools: yields
        (posteriors, debug dict with 'genotype_prior', 'genotype_addition'); the posteriors are a PooledPosteriors with pools and
        probs_df without, the yielded addition is the one the iteration's E-step used.  The EM state lives on the GPU between
        yields, in a device context private to this generator."""
        setup = Demultiplexer._doublet_learning_setup(genotypes, barcode_handler, doublet_prior, min_pair_posterior, barcode2pool, pool2donors,
                                                      'staged_genotype_learning_from_doublets')
        pools = (setup.pool_columns, setup.pool_of_barcode, doublet_prior != 0, setup.pair_penalty)

        with _generator_context() as ctx:
            _ctx, prior_betas = _pack_on_device(chromosome2compressed_snp_calls, genotypes, barcode_handler.n_barcodes, True, ctx=ctx)
            genotype_addition = np.zeros_like(prior_betas)
            ctx.set_addition(None)
            for _iteration in range(n_iterations):
                ctx.probs_from_betas(p_genotype_clip, fetch=False)
                out = ctx.estep_pools(*pools, fetch_logits=setup.pooled, resident=True)
                yield _framed_posteriors(setup, barcode_handler, out, None), {
                    'genotype_prior': prior_betas,
                    'genotype_addition': genotype_addition,
                }
                genotype_addition = ctx.mstep_doublets(*pools, out['probs'], min_pair_posterior, Demultiplexer.contribution_power)

    @staticmethod
    def _share_posteriors(setup, genotypes, barcode_handler, grid, log_weights, out):
        """The DoubletSharePosteriors of a pass over a grid of mixing shares (index name None: the learning entries' frames)."""
        names = list(genotypes.genotype_names)
        return DoubletSharePosteriors(barcode_handler.ordered_barcodes, setup.option_names, [[names[g] for g in columns] for columns in setup.pool_columns],
                                      setup.pool_of_barcode, out['row_ptr'], grid, log_weights, out['share_index'], out['share_mean'],
                                      out['best_option'], out['best_prob'], out['doublet_mass'], out['best_share_index'], out['best_share_mean'],
                                      _framed_posteriors(setup, barcode_handler, out, None), index_name=None)

    @staticmethod
    def learn_genotypes_with_doublet_shares(chromosome2compressed_snp_calls,
                                            genotypes,
                                            barcode_handler,
                                            n_iterations=5,
                                            p_genotype_clip=0.01,
                                            doublet_prior=0.35,
                                            shares=None,
                                            share_log_weights=None,
                                            min_pair_posterior=1e-3,
                                            barcode2pool=None,
                                            pool2donors=None) -> Tuple[object, DoubletSharePosteriors]:
        """(not in the reference) learn_genotypes_from_doublets for doublets of unequal shares: its loop with the E-step of
        predict_posteriors_with_doublet_shares - every pair option the marginal over a grid of mixing shares, so that an 80 / 20
        doublet is recognised at all - and an M-step that credits the donors of a pair 'A+B' at the pair's posterior mean share w of
        A: r_A = prob[A] w / (prob[A] w + prob[B] (1 - w)), r_B the rest, in place of the even mixture's prob[A] / (prob[A] + prob[B]),
        which hands the minor donor too much of the major donor's signal.  With shares=[0.5] and
        share_log_weights=[0.0] the result is learn_genotypes_from_doublets' bit for bit.  The whole loop runs on the GPU
        (dmx_em_doublet_shares); its sums are float64 in the reference's order whatever DEMUXALOT_AMD_ESTEP says.
        :param shares, share_log_weights: the grid and the prior over it, as predict_posteriors_with_doublet_shares takes them
            (None: 0.1 .. 0.9 under the uniform prior)
        :param min_pair_posterior, barcode2pool, pool2donors: as learn_genotypes_from_doublets takes them
        :return: learnt genotypes (betas = raw betas + the addition used by the last E-step) and the DoubletSharePosteriors of the
            last iteration.
        ValueError: what predict_posteriors_with_doublet_shares and learn_genotypes_from_doublets raise."""
        assert n_iterations >= 1, 'n_iterations should be positive'
        grid, log_weights = resolve_shares(shares, share_log_weights)
        setup = Demultiplexer._doublet_learning_setup(genotypes, barcode_handler, doublet_prior, min_pair_posterior, barcode2pool, pool2donors,
                                                      'learn_genotypes_with_doublet_shares')
        with shared_context_lock:
            ctx, _betas = _pack_on_device(chromosome2compressed_snp_calls, genotypes, barcode_handler.n_barcodes, True,
                                          fetch_betas=False)
            out = ctx.em_doublet_shares(n_iterations, p_genotype_clip, setup.pool_columns, setup.pool_of_barcode, doublet_prior != 0,
                                        setup.pair_penalty, grid, log_weights, min_pair_posterior,
                                        contribution_power=Demultiplexer.contribution_power, fetch_addition=False)
            learnt_betas = ctx.get_learnt_betas()  # genotypes.get_betas() + addition (demux.py:65), added on the device
        return genotypes._with_betas(learnt_betas, _take=True), Demultiplexer._share_posteriors(setup, genotypes, barcode_handler, grid, log_weights, out)

    @staticmethod
    def staged_genotype_learning_with_doublet_shares(chromosome2compressed_snp_calls,
                                                     genotypes,
                                                     barcode_handler,
                                                     n_iterations=5,
                                                     p_genotype_clip=0.01,
                                                     doublet_prior=0.35,
                                                     shares=None,
                                                     share_log_weights=None,
                                                     min_pair_posterior=1e-3,
                                                     barcode2pool=None,
                                                     pool2donors=None):
        """Generator over the iterations of learn_genotypes_with_doublet_shares, shaped like staged_genotype_learning_from_doublets:
        yields (DoubletSharePosteriors, debug dict with 'genotype_prior', 'genotype_addition'); the yielded addition is the one the
        iteration's E-step used.  The EM state lives on the GPU between yields, in a device context private to this generator."""
        grid, log_weights = resolve_shares(shares, share_log_weights)
        setup = Demultiplexer._doublet_learning_setup(genotypes, barcode_handler, doublet_prior, min_pair_posterior, barcode2pool, pool2donors,
                                                      'staged_genotype_learning_with_doublet_shares')
        pools = (setup.pool_columns, setup.pool_of_barcode, doublet_prior != 0, setup.pair_penalty)

        with _generator_context() as ctx:
            _ctx, prior_betas = _pack_on_device(chromosome2compressed_snp_calls, genotypes, barcode_handler.n_barcodes, True, ctx=ctx)
            genotype_addition = np.zeros_like(prior_betas)
            ctx.set_addition(None)
            for _iteration in range(n_iterations):
                ctx.probs_from_betas(p_genotype_clip, fetch=False)
                out = ctx.estep_pair_shares(*pools, grid, log_weights, resident=True)
                yield Demultiplexer._share_posteriors(setup, genotypes, barcode_handler, grid, log_weights, out), {
                    'genotype_prior': prior_betas,
                    'genotype_addition': genotype_addition,
                }
                genotype_addition = ctx.mstep_doublet_shares(*pools, out['probs'], out['share_mean'], min_pair_posterior,
                                                             Demultiplexer.contribution_power)

    # ------------------------------------------------------------------------------------
    @staticmethod
    def _doublet_penalties(n_genotypes: int, doublet_prior: float) -> np.ndarray:
        """Logit offsets of the K options (demux.py:158-173): zero for singlets; for pairs the log-odds
        that makes the prior doublet mass equal `doublet_prior` whatever the number of genotypes."""
        assert 0 <= doublet_prior < 1
        if doublet_prior == 0:
            return np.zeros(n_genotypes, dtype='float32')
        n_pair_slots = n_genotypes * max(n_genotypes - 1, 1) / 2
        bonus = np.log(n_genotypes * doublet_prior) - np.log(n_pair_slots * (1 - doublet_prior))
        penalties = np.zeros(n_genotypes * (n_genotypes + 1) // 2, dtype='float32')
        penalties[n_genotypes:] = bonus
        return penalties

    @staticmethod
    def _iterate_genotypes_options(genotype_names, genotype_prob: np.ndarray, doublet_prior: float):
        """Enumerates the K options as the reference does (demux.py:175-191): (index, column name,
        per-variant probability vector), singlets first, then pairs g1 < g2 row-major with
        (p1 + p2) * 0.5.  Kept for callers that inspect the options; the GPU kernels enumerate the same
        order internally and never call this."""
        k = 0
        for g, name in enumerate(genotype_names):
            yield k, name, genotype_prob[:, g]
            k += 1
        if doublet_prior != 0:
            assert doublet_prior > 0
            for g1, name1 in enumerate(genotype_names):
                for g2 in range(g1 + 1, len(genotype_names)):
                    yield k, f'{name1}+{genotype_names[g2]}', (genotype_prob[:, g1] + genotype_prob[:, g2]) * 0.5
                    k += 1

    @staticmethod
    def compute_barcode_logits(genotype_names, barcode_calls, molecule_calls, doublet_prior: float,
                               genotype_prob: np.ndarray, n_barcodes: int, n_genotypes: int):
        """Dispatcher of demux.py:193-202; with Demultiplexer.aggregate_on_snps the per-(barcode, SNP)
        regularised form of demux.py:204-244 over `molecule_calls` (float64 logits)."""
        if not Demultiplexer.aggregate_on_snps:
            return Demultiplexer.compute_barcode_logits_using_barcode_calls(
                genotype_names, barcode_calls=barcode_calls, doublet_prior=doublet_prior,
                genotype_prob=genotype_prob, n_barcodes=n_barcodes, n_genotypes=n_genotypes)
        genotype_prob = np.asarray(genotype_prob)
        assert genotype_prob.shape[1] == n_genotypes == len(genotype_names)
        n_variants = genotype_prob.shape[0]
        # SNP of every variant, from the molecule calls themselves (snp_id is a function of variant_id)
        v2snp = np.arange(n_variants, dtype=np.int32) + (int(np.max(molecule_calls['snp_id'])) + 1 if len(molecule_calls) else 0)
        v2snp[np.asarray(molecule_calls['variant_id'])] = molecule_calls['snp_id']
        with shared_context_lock:
            ctx = get_context()
            empty_i = np.zeros(0, dtype=np.int32)
            ctx.set_problem(n_barcodes, n_variants, n_genotypes, empty_i, empty_i, np.zeros(0, dtype=np.float32), v2snp)
            ctx.set_probs(genotype_prob)
            ctx.set_molecule_calls(molecule_calls['variant_id'], molecule_calls['compressed_cb'], molecule_calls['p_base_wrong'])
            logits, _ = ctx.estep_snp(doublet_prior != 0, Demultiplexer.compensation_during_computing_barcode_logits)
        return logits, _option_names(genotype_names, doublet_prior)

    @staticmethod
    def compute_barcode_logits_using_barcode_calls(genotype_names, barcode_calls, doublet_prior,
                                                   genotype_prob: np.ndarray, n_barcodes: int, n_genotypes: int):
        """E-step on caller-supplied tables (demux.py:246-265): barcode_calls carries the columns
        'variant_id', 'compressed_cb', 'p_base_wrong'; genotype_prob is float32[V, G]."""
        genotype_prob = np.asarray(genotype_prob)
        assert genotype_prob.shape[1] == n_genotypes == len(genotype_names)
        penalties = Demultiplexer._doublet_penalties(n_genotypes, doublet_prior=doublet_prior)
        with shared_context_lock:
            ctx = get_context()
            ctx.set_problem(n_barcodes, genotype_prob.shape[0], n_genotypes, barcode_calls['variant_id'],
                            barcode_calls['compressed_cb'], barcode_calls['p_base_wrong'],
                            np.zeros(genotype_prob.shape[0], dtype=np.int32))
            ctx.set_probs(genotype_prob)
            logits, _ = ctx.estep(penalties, with_doublets=doublet_prior != 0, fetch_probs=False)
        return logits, _option_names(genotype_names, doublet_prior)

    @staticmethod
    def _compute_probs_from_betas(variant_index2snp_index, variant_index2betas, p_genotype_clip):
        """P-step on caller-supplied tables (demux.py:267-274).  float32 betas take the EM path's kernel; any
        other dtype is carried as float64, as numpy's own promotion does (float64 division, one rounding)."""
        betas = np.asarray(variant_index2betas)
        as_f32 = betas.dtype == np.float32
        betas = np.ascontiguousarray(betas, dtype=np.float32 if as_f32 else np.float64)
        empty_i = np.zeros(0, dtype=np.int32)
        with shared_context_lock:
            ctx = get_context()
            ctx.set_problem(0, betas.shape[0], betas.shape[1], empty_i, empty_i, np.zeros(0, dtype=np.float32),
                            variant_index2snp_index)
            if not as_f32:
                return ctx.probs_from_betas_f64(betas, p_genotype_clip)
            ctx.set_betas(betas)
            ctx.set_addition(None)
            return ctx.probs_from_betas(p_genotype_clip)

    @staticmethod
    def molecule_calls2barcode_calls(molecule_calls, _prepacked=None):
        """Unique (variant, barcode) calls from matched molecule calls (demux.py:276-300), as the
        reference's record array (variant-major order)."""
        variant_id = np.ascontiguousarray(molecule_calls['variant_id'], dtype=np.int32)
        snp_id = np.ascontiguousarray(molecule_calls['snp_id'], dtype=np.int32)
        cb = np.ascontiguousarray(molecule_calls['compressed_cb'], dtype=np.int32)
        p = np.ascontiguousarray(molecule_calls['p_base_wrong'], dtype=np.float32)
        if _prepacked is None:
            # route the already-matched calls through the same host packer: key = variant row
            import ctypes
            lib = _lib.load()
            n = len(variant_id)
            n_variants = int(variant_id.max()) + 1 if n else 0
            rows = np.arange(n_variants, dtype=np.int32)
            zeros_v = np.zeros(n_variants, dtype=np.int32)
            zeros_b = np.zeros(n_variants, dtype=np.uint8)
            out_v, out_cb = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
            out_p, out_count = np.empty(n, dtype=np.float32), np.empty(n, dtype=np.int64)
            n_matched, n_unique = ctypes.c_int64(0), ctypes.c_int64(0)
            _lib.check(lib.dmx_pack_calls_host(
                n_variants, _lib.ptr(zeros_v), _lib.ptr(rows), _lib.ptr(zeros_b),
                n, _lib.ptr(np.zeros(n, dtype=np.int32)), _lib.ptr(variant_id), _lib.ptr(np.zeros(n, dtype=np.uint8)),
                _lib.ptr(cb), _lib.ptr(p), None, ctypes.byref(n_matched), ctypes.byref(n_unique),
                _lib.ptr(out_v), _lib.ptr(out_cb), _lib.ptr(out_p), _lib.ptr(out_count), None))
            k = n_unique.value
            u_variant, u_cb, u_p, u_count = out_v[:k].copy(), out_cb[:k].copy(), out_p[:k].copy(), out_count[:k].copy()
        else:
            u_variant, u_cb, u_p, u_count = _prepacked
        # snp id of a unique call: snp_id is a function of variant_id
        variant2snp = np.zeros(int(variant_id.max()) + 1 if len(variant_id) else 0, dtype=np.int32)
        variant2snp[variant_id] = snp_id
        u_snp = variant2snp[u_variant] if len(u_variant) else np.zeros(0, dtype=np.int32)
        # how many molecules of the barcode hit the SNP (any variant of it); nothing downstream reads it
        if len(u_variant):
            key = u_snp.astype(np.int64) * (int(u_cb.max()) + 1) + u_cb
            _, inverse = np.unique(key, return_inverse=True)
            snp_count = np.bincount(inverse, u_count)[inverse]
        else:
            snp_count = np.zeros(0, dtype=np.float64)
        return np.rec.fromarrays(
            [u_variant, u_snp, u_cb, u_p, u_count, snp_count],
            names=['variant_id', 'snp_id', 'compressed_cb', 'p_base_wrong', 'barcode_variant_count',
                   'barcode_snp_count'])

    @staticmethod
    def pack_calls(chromosome2compressed_snp_calls, genotypes, add_data_prior: bool):
        """demux.py:303-392: returns (variant_index2snp_index, regularised betas (read-only),
        matched molecule calls, unique barcode calls)."""
        from .snp_counter import split_call_sets
        if split_call_sets(chromosome2compressed_snp_calls):  # the public host twin: the records come to the host
            chromosome2compressed_snp_calls = {chrom: calls.to_host() for chrom, calls in chromosome2compressed_snp_calls.items()}
        packed = _pack(chromosome2compressed_snp_calls, genotypes, add_data_prior, want_molecule_table=True)
        barcode_calls = Demultiplexer.molecule_calls2barcode_calls(
            packed.molecule_calls,
            _prepacked=(packed.variant_id, packed.compressed_cb, packed.p_base_wrong, packed.variant_count))
        return packed.v2snp, packed.betas, packed.molecule_calls, barcode_calls
