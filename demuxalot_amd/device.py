"""Thin object wrapper over the dmx_ctx of libdemux_hip.so: one context = one GPU + one HIP
stream + one resident problem (calls CSR/CSC, beta tables, logits/posteriors)."""
import ctypes
import os
import threading

import numpy as np

from . import _lib
from ._lib import DMX_F32, DMX_F64, as_c, check, ptr
from .pools import pooled_layout


# E-step arithmetic of a new context (include/demux_hip.h: dmx_set_estep_mode); DEMUXALOT_AMD_ESTEP overrides.
# 'guarded': the contract of the path - assignments identical to the reference, posteriors within 1e-5 - PROVEN per barcode and
# E-step, every barcode that cannot be proven redone with the bit-exact kernel; E-steps that take the dictionary form (large
# singlet runs on the importers' genotype tables: predict_posteriors, EM iteration 0) stay bit-identical to the reference.
# 'exact': every logit, posterior and beta addition bit-identical to the reference, at 1.6x the time per EM iteration.
DEFAULT_ESTEP_MODE = 'guarded'


class DeviceContext:
    def __init__(self, device=0):
        self._lib = _lib.load()
        handle = ctypes.c_void_p()
        check(self._lib.dmx_create(int(device), ctypes.byref(handle)))
        self._h = handle
        self.device = int(device)
        self.B = self.V = self.G = self.N = 0
        self.K = 0
        self._resident_key = None
        self._keep_molecule_calls = False
        self._snp_shape = (0, 0)
        self.apply_environment()

    def apply_environment(self):
        """The modes the environment selects (also re-applied when a pooled context is handed out again):
        DEMUXALOT_AMD_ESTEP = exact | guarded | fast (dmx_set_estep_mode); DEMUXALOT_AMD_EXACT_ADDITIONS = 1 | 0: the
        bit-identical genotype additions of the hottest variants (several work items) cost ~4 % per EM iteration
        (include/demux_hip.h: dmx_set_exact_additions; default: with the exact E-step); DEMUXALOT_AMD_ESTEP_SCHEDULE = direct | auto | tiled
        (dmx_set_estep_schedule); DEMUXALOT_AMD_ESTEP_DICT = never | auto | always (dmx_set_estep_dictionary);
        DEMUXALOT_AMD_ESTEP_PACKED = never | auto | always (dmx_set_estep_packing); DEMUXALOT_AMD_COARSE_PASS = 1 | 0: the guarded
        mode's binary16 pass for E-steps whose logits nobody reads (dmx_set_coarse_pass; default on); DEMUXALOT_AMD_MSTEP_INCREMENTAL
        = 1 | 0: the tile-major M-step keeps its integer sums and adds differences (dmx_set_mstep_incremental; default on);
        DEMUXALOT_AMD_LEAN = 0 | 1: release the fine pass's copy of the E-step records once the coarse pass's are built (dmx_set_lean_memory);
        DEMUXALOT_AMD_LIVE_FLOOR_GRID = 1 | 0: barcode codes at the fixed-point M-step's live floor (dmx_set_live_floor_on_grid; default on)."""
        mode = os.environ.get('DEMUXALOT_AMD_ESTEP', '') or DEFAULT_ESTEP_MODE
        assert mode in ('exact', 'fast', 'guarded'), f'DEMUXALOT_AMD_ESTEP={mode!r}: exact, fast or guarded'
        self.set_estep_mode(mode)
        # the M-step's exact summation keeps the additions bit-identical to the reference GIVEN bit-identical posteriors:
        # it goes with the exact E-step unless asked for
        exact_additions = os.environ.get('DEMUXALOT_AMD_EXACT_ADDITIONS', '')
        self.set_exact_additions(mode == 'exact' if exact_additions == '' else exact_additions != '0')
        self.set_estep_schedule(os.environ.get('DEMUXALOT_AMD_ESTEP_SCHEDULE', 'auto'))
        self.set_estep_dictionary(os.environ.get('DEMUXALOT_AMD_ESTEP_DICT', 'auto'))
        self.set_estep_packing(os.environ.get('DEMUXALOT_AMD_ESTEP_PACKED', 'auto'))
        self.set_coarse_pass(os.environ.get('DEMUXALOT_AMD_COARSE_PASS', '1') != '0')
        self.set_mstep_incremental(os.environ.get('DEMUXALOT_AMD_MSTEP_INCREMENTAL', '1') != '0')
        self.set_lean_memory(os.environ.get('DEMUXALOT_AMD_LEAN', '0') not in ('', '0'))
        self.set_live_floor_on_grid(os.environ.get('DEMUXALOT_AMD_LIVE_FLOOR_GRID', '1') != '0')
        self.set_phase_timers(False)
        self.set_logits_needed(True)

    def __enter__(self):
        return self

    def __exit__(self, *_exc):
        self.close()

    def close(self):
        if getattr(self, '_h', None):
            self._lib.dmx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- problem ----------------------------------------------------------------------
    def set_problem(self, n_barcodes, n_variants, n_genotypes, variant_id, compressed_cb, p_base_wrong, v2snp):
        self._resident_key = None  # (demux.py: _pack_on_device keeps the packed problem of the shared context across calls)
        variant_id = as_c(variant_id, np.int32)
        compressed_cb = as_c(compressed_cb, np.int32)
        p_base_wrong = as_c(p_base_wrong, np.float32)
        v2snp = as_c(v2snp, np.int32)
        assert len(variant_id) == len(compressed_cb) == len(p_base_wrong)
        assert len(v2snp) == n_variants
        check(self._lib.dmx_set_problem(self._h, n_barcodes, n_variants, n_genotypes, len(variant_id),
                                        ptr(variant_id), ptr(compressed_cb), ptr(p_base_wrong), ptr(v2snp)))
        self.B, self.V, self.G, self.N = int(n_barcodes), int(n_variants), int(n_genotypes), len(variant_id)

    @staticmethod
    def _variant_arrays(var_chrom, var_pos, var_base, v2snp):
        """The variants of a pack as the ABI's arrays: (var_chrom, var_pos, var_base, v2snp)."""
        var_chrom, var_pos, var_base = as_c(var_chrom, np.int32), as_c(var_pos, np.int32), as_c(var_base, np.uint8)
        v2snp = as_c(v2snp, np.int32)
        assert len(v2snp) == len(var_pos)
        return var_chrom, var_pos, var_base, v2snp

    def _pack(self, entry, n_barcodes, n_genotypes, variants, *calls):
        """One of the dmx_pack_*_and_set_problem entry points on `variants` (_variant_arrays) and its own description of the
        calls; the packed problem becomes the resident one.  Returns (n_matched, n_unique, molecules per variant)."""
        n_variants = len(variants[1])
        mol_per_variant = np.zeros(n_variants, dtype=np.int64)
        n_matched, n_unique = ctypes.c_int64(0), ctypes.c_int64(0)
        check(entry(self._h, n_barcodes, n_variants, n_genotypes, *(ptr(a) for a in variants), *calls,
                    ctypes.byref(n_matched), ctypes.byref(n_unique), ptr(mol_per_variant)))
        self.B, self.V, self.G, self.N = int(n_barcodes), int(n_variants), int(n_genotypes), n_unique.value
        return n_matched.value, n_unique.value, mol_per_variant

    def pack_and_set_problem(self, n_barcodes, n_genotypes, var_chrom, var_pos, var_base, v2snp,
                             call_chrom, call_pos, call_base, call_cb, call_p):
        """Device pack (variant matching + de-duplication, demux.py:276-300, 332-365) installed directly as
        the resident problem. Returns (n_matched, n_unique, molecules per variant)."""
        self._resident_key = None  # (demux.py: _pack_on_device keeps the packed problem of the shared context across calls)
        variants = self._variant_arrays(var_chrom, var_pos, var_base, v2snp)
        call_chrom, call_pos = as_c(call_chrom, np.int32), as_c(call_pos, np.int32)
        call_base, call_cb, call_p = as_c(call_base, np.uint8), as_c(call_cb, np.int32), as_c(call_p, np.float32)
        return self._pack(self._lib.dmx_pack_and_set_problem, n_barcodes, n_genotypes, variants, len(call_pos),
                          ptr(call_chrom), ptr(call_pos), ptr(call_base), ptr(call_cb), ptr(call_p))

    def _container_list(self, containers):
        from .snp_counter import MOLECULE_DTYPE, SNP_CALL_DTYPE

        class Container(ctypes.Structure):
            _fields_ = [('snp_calls', ctypes.c_void_p), ('n_snp_calls', ctypes.c_int64),
                        ('molecules', ctypes.c_void_p), ('n_molecules', ctypes.c_int64), ('chrom', ctypes.c_int32)]

        keep_alive, parts = [], (Container * max(1, len(containers)))()
        for k, (chrom, snp_calls, molecules) in enumerate(containers):
            assert snp_calls.dtype == SNP_CALL_DTYPE and molecules.dtype == MOLECULE_DTYPE
            snp_calls, molecules = np.ascontiguousarray(snp_calls), np.ascontiguousarray(molecules)
            keep_alive += [snp_calls, molecules]
            parts[k] = Container(snp_calls.ctypes.data, len(snp_calls), molecules.ctypes.data, len(molecules), int(chrom))
        return parts, keep_alive

    def pack_containers_and_set_problem(self, n_barcodes, n_genotypes, var_chrom, var_pos, var_base, v2snp, containers):
        """pack_and_set_problem fed with the raw record arrays of the call containers:
        `containers` = [(chromosome index, snp_calls[:n] (SNP_CALL_DTYPE), molecules[:m] (MOLECULE_DTYPE))].
        The field extraction and the molecule -> barcode lookup happen on the GPU."""
        self._resident_key = None  # (demux.py: _pack_on_device keeps the packed problem of the shared context across calls)
        variants = self._variant_arrays(var_chrom, var_pos, var_base, v2snp)
        parts, _keep_alive = self._container_list(containers)
        return self._pack(self._lib.dmx_pack_containers_and_set_problem, n_barcodes, n_genotypes, variants,
                          ctypes.cast(parts, ctypes.c_void_p), len(containers))

    def stage_containers(self, containers):
        """First half of pack_containers_and_set_problem: upload + field extraction of the containers' records, which
        needs nothing of the genotypes (`containers` as there, the chromosome index provisional: the position in the
        list).  The resident problem stays as it is.  include/demux_hip.h: dmx_stage_containers."""
        self._resident_key = None  # (demux.py: _pack_on_device keeps the packed problem of the shared context across calls)
        parts, _keep_alive = self._container_list(containers)
        check(self._lib.dmx_stage_containers(self._h, ctypes.cast(parts, ctypes.c_void_p), len(containers)))

    def pack_staged_and_set_problem(self, n_barcodes, n_genotypes, var_chrom, var_pos, var_base, v2snp, chrom_of_container):
        """Second half: variant matching, de-duplication and layouts on the staged calls.  chrom_of_container[k] = the
        chromosome index (numbering of var_chrom) of the k-th staged container, -1 when no variant lies on it."""
        self._resident_key = None  # (demux.py: _pack_on_device keeps the packed problem of the shared context across calls)
        variants = self._variant_arrays(var_chrom, var_pos, var_base, v2snp)
        table = as_c(chrom_of_container, np.int32)
        return self._pack(self._lib.dmx_pack_staged_and_set_problem, n_barcodes, n_genotypes, variants, ptr(table), len(table))

    def get_packed_calls(self):
        """Unique (variant, barcode) calls left on the device by pack_and_set_problem, variant-major."""
        n = self.N
        variant, cb = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        p, count = np.empty(n, dtype=np.float32), np.empty(n, dtype=np.int64)
        check(self._lib.dmx_get_packed_calls(self._h, ptr(variant), ptr(cb), ptr(p), ptr(count)))
        return variant, cb, p, count

    def set_betas(self, betas):
        betas = as_c(betas, np.float32)
        assert betas.shape == (self.V, self.G)
        check(self._lib.dmx_set_betas(self._h, ptr(betas)))

    def set_prior_betas(self, raw_betas, default_prior, add_data_prior, mol_per_variant=None, fetch=True):
        """Regularised prior betas (demux.py:372-388) computed on the GPU from the raw betas."""
        raw_betas = as_c(raw_betas, np.float32)
        assert raw_betas.shape == (self.V, self.G)
        assert np.all(raw_betas >= 0), 'bad genotypes provided, negative betas appeared'
        if mol_per_variant is not None:
            mol_per_variant = as_c(mol_per_variant, np.int64)
            assert mol_per_variant.shape == (self.V,)
        out = np.empty((self.V, self.G), dtype=np.float32) if fetch else None
        check(self._lib.dmx_set_prior_betas(self._h, ptr(raw_betas), float(default_prior), int(bool(add_data_prior)),
                                            ptr(mol_per_variant), ptr(out)))
        if out is not None:
            out.flags.writeable = False
        return out

    def set_addition(self, addition=None):
        if addition is not None:
            addition = as_c(addition, np.float32)
            assert addition.shape == (self.V, self.G)
        check(self._lib.dmx_set_addition(self._h, ptr(addition)))

    def set_probs(self, prob):
        prob = as_c(prob, np.float32)
        assert prob.shape == (self.V, self.G)
        check(self._lib.dmx_set_probs(self._h, ptr(prob)))

    # ---- steps ------------------------------------------------------------------------
    @staticmethod
    def clip_bounds(p_genotype_clip):
        # ndarray.clip(p, 1 - p) on a float32 array: both Python floats become float32 scalars
        return float(np.float32(p_genotype_clip)), float(np.float32(1 - p_genotype_clip))

    def probs_from_betas(self, p_genotype_clip, fetch=True):
        lo, hi = self.clip_bounds(p_genotype_clip)
        out = np.empty((self.V, self.G), dtype=np.float32) if fetch else None
        check(self._lib.dmx_probs_from_betas(self._h, lo, hi, ptr(out)))
        return out

    def probs_from_betas_f64(self, betas, p_genotype_clip):
        """P-step on caller-supplied float64 betas (dmx_probs_from_betas_f64)."""
        betas = as_c(betas, np.float64)
        assert betas.shape == (self.V, self.G)
        lo, hi = self.clip_bounds(p_genotype_clip)
        out = np.empty((self.V, self.G), dtype=np.float32)
        check(self._lib.dmx_probs_from_betas_f64(self._h, ptr(betas), lo, hi, ptr(out)))
        return out

    def _n_options(self, with_doublets):
        return self.G * (self.G + 1) // 2 if with_doublets else self.G

    @staticmethod
    def _prior_arg(prior_logits, shape):
        if prior_logits is None:
            return None, DMX_F32
        prior_logits = np.asarray(prior_logits)
        assert prior_logits.shape == shape, 'mismatching priors passed'
        if prior_logits.dtype == np.float32:
            return as_c(prior_logits, np.float32), DMX_F32
        # any other dtype takes numpy's float64 path of `logits += prior`
        return as_c(prior_logits, np.float64), DMX_F64

    def estep(self, penalties, with_doublets, prior_logits=None, fetch_logits=True, fetch_probs=True):
        K = self._n_options(with_doublets)
        penalties = as_c(penalties, np.float32)
        assert penalties.shape == (K,)
        prior, prior_dtype = self._prior_arg(prior_logits, (self.B, K))
        logits = np.empty((self.B, K), dtype=np.float32) if fetch_logits else None
        probs = np.empty((self.B, K), dtype=np.float32) if fetch_probs else None
        check(self._lib.dmx_estep(self._h, int(with_doublets), ptr(penalties), ptr(prior), prior_dtype,
                                  ptr(logits), ptr(probs)))
        self.K = K
        return logits, probs

    def mstep(self, contribution_power=2., fetch=True):
        out = np.empty((self.V, self.G), dtype=np.float32) if fetch else None
        check(self._lib.dmx_mstep(self._h, float(contribution_power), ptr(out)))
        return out

    def em(self, n_iterations, p_genotype_clip, penalties, with_doublets, prior_logits=None,
           contribution_power=2., fetch_logits=True, fetch_probs=True, fetch_addition=True):
        K = self._n_options(with_doublets)
        lo, hi = self.clip_bounds(p_genotype_clip)
        penalties = as_c(penalties, np.float32)
        assert penalties.shape == (K,)
        prior, prior_dtype = self._prior_arg(prior_logits, (self.B, K))
        logits = np.empty((self.B, K), dtype=np.float32) if fetch_logits else None
        probs = np.empty((self.B, K), dtype=np.float32) if fetch_probs else None
        addition = np.empty((self.V, self.G), dtype=np.float32) if fetch_addition else None
        check(self._lib.dmx_em(self._h, int(n_iterations), lo, hi, int(with_doublets), ptr(penalties), ptr(prior),
                               prior_dtype, float(contribution_power), ptr(logits), ptr(probs), ptr(addition)))
        self.K = K
        return logits, probs, addition

    def run_iterations(self, n_iterations, p_genotype_clip, contribution_power=2.):
        """Enqueue n full EM iterations (P, E, M) without synchronising; see dmx_run_iterations."""
        lo, hi = self.clip_bounds(p_genotype_clip)
        check(self._lib.dmx_run_iterations(self._h, int(n_iterations), lo, hi, float(contribution_power)))

    def get_logits(self):
        out = np.empty((self.B, self.K), dtype=np.float32)
        check(self._lib.dmx_get_logits(self._h, ptr(out)))
        return out

    def get_probs(self):
        out = np.empty((self.B, self.K), dtype=np.float32)
        check(self._lib.dmx_get_probs(self._h, ptr(out)))
        return out

    def get_addition(self):
        out = np.empty((self.V, self.G), dtype=np.float32)
        check(self._lib.dmx_get_addition(self._h, ptr(out)))
        return out

    def get_block(self, what, b0=0, b1=None, k0=0, k1=None):
        """Rows [b0, b1) x columns [k0, k1) of the resident 'logits' or 'probs' (dmx_get_block)."""
        b1 = self.B if b1 is None else b1
        k1 = self.K if k1 is None else k1
        out = np.empty((b1 - b0, k1 - k0), dtype=np.float32)
        check(self._lib.dmx_get_block(self._h, {'logits': 0, 'probs': 1}[what], b0, b1, k0, k1, ptr(out)))
        return out

    def get_assignments(self):
        best = np.empty(self.B, dtype=np.int32)
        prob = np.empty(self.B, dtype=np.float32)
        check(self._lib.dmx_get_assignments(self._h, ptr(best), ptr(prob)))
        return best, prob

    # ---- aggregate_on_snps (demux.py:204-244) --------------------------------------------------------
    def set_keep_molecule_calls(self, keep):
        self._keep_molecule_calls = bool(keep)
        check(self._lib.dmx_set_keep_molecule_calls(self._h, int(bool(keep))))

    def set_molecule_calls(self, variant_id, compressed_cb, p_base_wrong):
        self._resident_key = None  # (demux.py: _pack_on_device keeps the packed problem of the shared context across calls)
        variant_id, compressed_cb = as_c(variant_id, np.int32), as_c(compressed_cb, np.int32)
        p_base_wrong = as_c(p_base_wrong, np.float32)
        assert len(variant_id) == len(compressed_cb) == len(p_base_wrong)
        check(self._lib.dmx_set_molecule_calls(self._h, len(variant_id), ptr(variant_id), ptr(compressed_cb), ptr(p_base_wrong)))

    def estep_snp(self, with_doublets, compensation, prior_logits=None):
        """E-step of aggregate_on_snps: (logits float64[B, K], posteriors float64[B, K])."""
        K = self._n_options(with_doublets)
        n = ctypes.c_int64(0)
        check(self._lib.dmx_get_max_pair_count(self._h, ctypes.byref(n)))
        # `counts[:, None] ** compensation` of demux.py:232 for every count that occurs, evaluated by numpy itself
        # on an int64 array like the reference's, so that its pow() is repeated to the last bit
        count_pow = np.ascontiguousarray(np.arange(n.value + 1, dtype=np.int64) ** compensation, dtype=np.float64)
        prior, prior_dtype = self._prior_arg(prior_logits, (self.B, K))
        logits = np.empty((self.B, K), dtype=np.float64)
        probs = np.empty((self.B, K), dtype=np.float64)
        check(self._lib.dmx_estep_snp(self._h, int(with_doublets), ptr(count_pow), len(count_pow), ptr(prior), prior_dtype,
                                      ptr(logits), ptr(probs)))
        self.K = K
        return logits, probs

    def mstep_f64(self, contribution_power=2., as_float64=False):
        """M-step on the float64 posteriors of estep_snp.  as_float64: the unrounded float64 sums (a barcode-sharded run
        adds them over ranks before the one float32 rounding)."""
        if as_float64:
            out = np.empty((self.V, self.G), dtype=np.float64)
            check(self._lib.dmx_mstep_f64_sums(self._h, float(contribution_power), ptr(out)))
            return out
        out = np.empty((self.V, self.G), dtype=np.float32)
        check(self._lib.dmx_mstep_f64(self._h, float(contribution_power), ptr(out)))
        return out

    def get_prior_betas(self):
        out = np.empty((self.V, self.G), dtype=np.float32)
        check(self._lib.dmx_get_prior_betas(self._h, ptr(out)))
        out.flags.writeable = False
        return out

    def get_learnt_betas(self):
        """raw betas (as given to set_prior_betas) + the last M-step's addition, float32 [V, G], added on the device
        (include/demux_hip.h: dmx_get_learnt_betas; demux.py:65)."""
        out = np.empty((self.V, self.G), dtype=np.float32)
        check(self._lib.dmx_get_learnt_betas(self._h, ptr(out)))
        return out

    def get_assignments_above(self, threshold):
        """(best option or -1 where the row maximum is not > threshold, row maximum, number assigned)."""
        best = np.empty(self.B, dtype=np.int32)
        prob = np.empty(self.B, dtype=np.float32)
        n = ctypes.c_int64(0)
        check(self._lib.dmx_get_assignments_above(self._h, float(threshold), ptr(best), ptr(prob), ctypes.byref(n)))
        return best, prob, n.value

    # ---- SNP detection (include/demux_hip.h: dmx_snp_count / _score / _select; demuxalot_amd/snp_detection.py) ----
    def snp_count(self, containers, donor_of_barcode, n_donors, p_threshold=0.01, cap=3):
        """Counts [position, donor, base] of the calls in `containers` ([(chrom number, snp_calls, molecules)] as for
        pack_containers_and_set_problem) on the device; returns the number of positions.  The resident problem stays."""
        parts, _keep_alive = self._container_list(containers)
        donor_of_barcode = as_c(donor_of_barcode, np.int32)
        n = ctypes.c_int64(0)
        check(self._lib.dmx_snp_count(self._h, ctypes.cast(parts, ctypes.c_void_p), len(containers), ptr(donor_of_barcode),
                                      len(donor_of_barcode), int(n_donors), float(np.float32(p_threshold)), int(cap),
                                      ctypes.byref(n)))
        self._snp_shape = (n.value, int(n_donors))
        return n.value

    def snp_score(self, regularization, fetch_counts=True, fetch_importances=True):
        """dict chrom, pos (int32[P]), counts (int32[P, D, 4]), importances (float64[P, D]), bases (uint8[P, 2]: ref, alt),
        base_totals (int64[P, 2]) of the last snp_count; counts / importances None unless fetched."""
        P, D = self._snp_shape
        out = dict(chrom=np.empty(P, np.int32), pos=np.empty(P, np.int32), bases=np.empty((P, 2), np.uint8),
                   base_totals=np.empty((P, 2), np.int64),
                   counts=np.empty((P, D, 4), np.int32) if fetch_counts else None,
                   importances=np.empty((P, D), np.float64) if fetch_importances else None)
        check(self._lib.dmx_snp_score(self._h, float(regularization), ptr(out['chrom']), ptr(out['pos']), ptr(out['counts']),
                                      ptr(out['importances']), ptr(out['bases']), ptr(out['base_totals'])))
        return out

    def snp_select(self, n_best_per_donor, n_additional):
        """Selected position indices (int64, ascending) of the last snp_score."""
        selected = np.empty(max(1, self._snp_shape[0]), dtype=np.int64)
        n = ctypes.c_int64(0)
        check(self._lib.dmx_snp_select(self._h, int(n_best_per_donor), int(n_additional), ptr(selected), ctypes.byref(n)))
        return selected[:n.value].copy()

    # ---- read counting (include/demux_hip.h: dmx_count_reads / _fetch; demuxalot_amd/snp_counter.py) ----
    @staticmethod
    def _reads_descriptor(reads, coverage_only=False):
        """(pointer to the dmx_decoded_reads of a DecodedReads, what must stay alive until the call returns); coverage_only
        leaves out the four columns only counting reads (compressed_cb, compressed_ub, p_misaligned, alignment_score)."""
        arrays = reads.arrays()  # C-contiguous arrays of the ABI's dtypes
        pointers = {name: ptr(a) for name, a in arrays.items()}
        if coverage_only:
            for name in ('compressed_cb', 'compressed_ub', 'p_misaligned', 'alignment_score'):
                pointers[name] = None
        desc = _lib.DecodedReadsStruct(n_reads=reads.n_reads, n_cigar_ops=len(arrays['cigar']), n_bases=len(arrays['seq']), **pointers)
        return ctypes.cast(ctypes.byref(desc), ctypes.c_void_p), (desc, arrays)

    @staticmethod
    def _count_inputs(positions, qual_table):
        positions = as_c(positions, np.int32)
        qual_table = as_c(qual_table, np.float64)
        assert qual_table.shape == (41,), 'qual_table holds the qualities 0 .. 40'
        return positions, qual_table

    def _counted(self, entry, *args, fetch=True):
        """(molecules, snp_calls) of a counting entry point: the call reports how many there are, dmx_count_reads_fetch copies them.
        fetch=False: (n_molecules, n_snp_calls), the records stay on the device (calls_append_counted takes them from there)."""
        from .snp_counter import MOLECULE_DTYPE, SNP_CALL_DTYPE
        n_molecules, n_calls = ctypes.c_int64(0), ctypes.c_int64(0)
        check(entry(self._h, *args, ctypes.byref(n_molecules), ctypes.byref(n_calls)))
        if not fetch:
            return n_molecules.value, n_calls.value
        molecules = np.empty(n_molecules.value, dtype=MOLECULE_DTYPE)
        snp_calls = np.empty(n_calls.value, dtype=SNP_CALL_DTYPE)
        check(self._lib.dmx_count_reads_fetch(self._h, ptr(molecules), ptr(snp_calls)))
        return molecules, snp_calls

    def count_reads(self, reads, positions, qual_table, fetch=True):
        """(molecules, snp_calls) structured arrays (snp_counter.MOLECULE_DTYPE / SNP_CALL_DTYPE) counted on the device from a
        DecodedReads at the strictly ascending int32 `positions`; qual_table float64[41].  The resident problem stays.
        fetch=False (here and in the three calls below): (n_molecules, n_snp_calls), the records stay on the device."""
        positions, qual_table = self._count_inputs(positions, qual_table)
        desc, _keep_alive = self._reads_descriptor(reads)
        return self._counted(self._lib.dmx_count_reads, desc, ptr(positions), len(positions), ptr(qual_table), fetch=fetch)

    def count_reads_timings(self):
        """{stage: milliseconds} of the last count_reads or count_reads_push (include/demux_hip_debug.h: dmx_get_count_reads_timings)."""
        ms = (ctypes.c_double * len(_lib.COUNT_READS_STAGES))()
        check(self._lib.dmx_get_count_reads_timings(self._h, ms))
        return dict(zip(_lib.COUNT_READS_STAGES, ms))

    # streamed (dmx_count_reads_begin / _push / _end; snp_counter.ReadCounter is the front)
    def count_reads_begin(self, positions, qual_table):
        positions, qual_table = self._count_inputs(positions, qual_table)
        check(self._lib.dmx_count_reads_begin(self._h, ptr(positions), len(positions), ptr(qual_table)))

    def count_reads_push(self, reads, final=False, fetch=True):
        """(molecules, snp_calls) this push emitted, molecule_index counting on across the stream; reads: a DecodedReads or None."""
        desc, _keep_alive = (None, None) if reads is None else self._reads_descriptor(reads)
        return self._counted(self._lib.dmx_count_reads_push, desc, 1 if final else 0, fetch=fetch)

    def count_reads_end(self):
        check(self._lib.dmx_count_reads_end(self._h))

    def count_reads_carry(self):
        """Reads the last push of the open stream left on the device (include/demux_hip_debug.h: dmx_get_count_reads_carry)."""
        n = ctypes.c_int64(0)
        check(self._lib.dmx_get_count_reads_carry(self._h, ctypes.byref(n)))
        return n.value

    def count_reads_peak_bytes(self):
        """Device bytes the last count_reads or count_reads_push held (include/demux_hip_debug.h: dmx_get_count_reads_peak_bytes)."""
        n = ctypes.c_int64(0)
        check(self._lib.dmx_get_count_reads_peak_bytes(self._h, ctypes.byref(n)))
        return n.value

    # ---- resident reads (include/demux_hip_debug.h "Resident reads"; snp_counter.ResidentReads is the front) ----
    def reads_upload(self, reads, coverage_only=False):
        """Handle of the DecodedReads' arrays uploaded once to this context; coverage_only leaves out the four columns only
        counting reads (compressed_cb, compressed_ub, p_misaligned, alignment_score)."""
        desc, _keep_alive = self._reads_descriptor(reads, coverage_only)
        handle = ctypes.c_int64(0)
        check(self._lib.dmx_reads_upload(self._h, desc, ctypes.byref(handle)))
        return handle.value

    def reads_release(self, handle):
        check(self._lib.dmx_reads_release(self._h, int(handle)))

    def reads_info(self, handle):
        """{n_reads, n_cigar_ops, n_bases, nbytes, reference_length} of a resident set (dmx_reads_info)."""
        info = (ctypes.c_int64 * len(_lib.READS_INFO))()
        check(self._lib.dmx_reads_info(self._h, int(handle), info))
        return dict(zip(_lib.READS_INFO, (int(v) for v in info)))

    def reads_upload_bytes(self):
        """Bytes of decoded-read arrays this context has copied host to device so far (dmx_get_reads_upload_bytes)."""
        n = ctypes.c_int64(0)
        check(self._lib.dmx_get_reads_upload_bytes(self._h, ctypes.byref(n)))
        return n.value

    def count_reads_resident(self, handle, positions, qual_table, fetch=True):
        """count_reads on a resident set."""
        positions, qual_table = self._count_inputs(positions, qual_table)
        return self._counted(self._lib.dmx_count_reads_resident, int(handle), ptr(positions), len(positions), ptr(qual_table), fetch=fetch)

    def count_reads_push_resident(self, handle, first_read, last_read, final=False, fetch=True):
        """count_reads_push with the reads [first_read, last_read) of a resident set as the chunk."""
        return self._counted(self._lib.dmx_count_reads_push_resident, int(handle), int(first_read), int(last_read), 1 if final else 0,
                             fetch=fetch)

    # ---- resident calls (include/demux_hip_debug.h "Resident calls"; snp_counter.ResidentCalls is the front) ----
    def calls_upload(self, snp_calls, molecules):
        """Handle of a sealed set holding copies of the two record arrays (SNP_CALL_DTYPE / MOLECULE_DTYPE) of one container."""
        parts, _keep_alive = self._container_list([(0, snp_calls, molecules)])
        handle = ctypes.c_int64(0)
        check(self._lib.dmx_calls_upload(self._h, ctypes.cast(parts, ctypes.c_void_p), ctypes.byref(handle)))
        return handle.value

    def calls_open(self):
        """Handle of a new, empty, open set (calls_append_counted fills it, calls_seal closes it)."""
        handle = ctypes.c_int64(0)
        check(self._lib.dmx_calls_open(self._h, ctypes.byref(handle)))
        return handle.value

    def calls_append_counted(self, handle):
        """Appends the records of the last count_reads / count_reads_push (any of the four) of this context, device to device."""
        check(self._lib.dmx_calls_append_counted(self._h, int(handle)))

    def calls_seal(self, handle):
        check(self._lib.dmx_calls_seal(self._h, int(handle)))

    def calls_concatenate(self, handles):
        """Handle of a new sealed set: the sets in list order, molecule_index shifted by the molecules before each."""
        handles = as_c(list(handles), np.int64)
        out = ctypes.c_int64(0)
        check(self._lib.dmx_calls_concatenate(self._h, handles.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(handles), ctypes.byref(out)))
        return out.value

    def calls_view(self, handle):
        """_lib.CallContainerStruct with the device pointers and sizes of a sealed set (chrom 0)."""
        view = _lib.CallContainerStruct()
        check(self._lib.dmx_calls_view(self._h, int(handle), ctypes.cast(ctypes.byref(view), ctypes.c_void_p)))
        return view

    def calls_info(self, handle):
        """{n_molecules, n_snp_calls, nbytes, sealed} of a set (dmx_calls_info)."""
        info = (ctypes.c_int64 * len(_lib.CALLS_INFO))()
        check(self._lib.dmx_calls_info(self._h, int(handle), info))
        return dict(zip(_lib.CALLS_INFO, (int(v) for v in info)))

    def calls_fetch(self, handle):
        """(molecules, snp_calls) structured arrays of a sealed set."""
        from .snp_counter import MOLECULE_DTYPE, SNP_CALL_DTYPE
        info = self.calls_info(handle)
        molecules = np.empty(info['n_molecules'], dtype=MOLECULE_DTYPE)
        snp_calls = np.empty(info['n_snp_calls'], dtype=SNP_CALL_DTYPE)
        check(self._lib.dmx_calls_fetch(self._h, int(handle), ptr(molecules), ptr(snp_calls)))
        return molecules, snp_calls

    def calls_release(self, handle):
        check(self._lib.dmx_calls_release(self._h, int(handle)))

    def calls_barcode_counts(self, handle, n_barcodes):
        """(calls int64[B], molecules int64[B]) per compressed_cb of a sealed set (dmx_calls_barcode_counts)."""
        calls, molecules = np.zeros(int(n_barcodes), dtype=np.int64), np.zeros(int(n_barcodes), dtype=np.int64)
        check(self._lib.dmx_calls_barcode_counts(self._h, int(handle), int(n_barcodes), ptr(calls), ptr(molecules)))
        return calls, molecules

    @staticmethod
    def _view_list(views):
        """[(chromosome number, CallContainerStruct view)] as the array of dmx_call_container the device entry points take."""
        parts = (_lib.CallContainerStruct * max(1, len(views)))()
        for k, (chrom, view) in enumerate(views):
            parts[k] = _lib.CallContainerStruct(view.snp_calls, view.n_snp_calls, view.molecules, view.n_molecules, int(chrom))
        return parts

    def stage_device_containers(self, views):
        """stage_containers from views of sealed resident call sets ([(provisional chromosome number, view)]): nothing is uploaded.
        The sets may belong to another context of this device.  include/demux_hip_debug.h: dmx_stage_device_containers."""
        self._resident_key = None  # (demux.py: _pack_on_device keeps the packed problem of the shared context across calls)
        parts = self._view_list(views)
        check(self._lib.dmx_stage_device_containers(self._h, ctypes.cast(parts, ctypes.c_void_p), len(views)))

    def snp_count_device(self, views, donor_of_barcode, n_donors, p_threshold=0.01, cap=3):
        """snp_count from views of sealed resident call sets ([(chromosome number, view)]); nothing of the calls is uploaded."""
        parts = self._view_list(views)
        donor_of_barcode = as_c(donor_of_barcode, np.int32)
        n = ctypes.c_int64(0)
        check(self._lib.dmx_snp_count_device(self._h, ctypes.cast(parts, ctypes.c_void_p), len(views), ptr(donor_of_barcode),
                                             len(donor_of_barcode), int(n_donors), float(np.float32(p_threshold)), int(cap),
                                             ctypes.byref(n)))
        self._snp_shape = (n.value, int(n_donors))
        return n.value

    def calls_transfer_bytes(self):
        """(host to device, device to host): bytes of call records this context has copied so far (dmx_get_calls_transfer_bytes)."""
        n = (ctypes.c_int64 * 2)()
        check(self._lib.dmx_get_calls_transfer_bytes(self._h, n))
        return int(n[0]), int(n[1])

    def coverage_count_resident(self, handle, start, stop, quality_threshold=15, fetch=True):
        """coverage_count on a resident set."""
        out = np.empty((4, max(0, int(stop) - int(start))), dtype=np.int32) if fetch else None
        check(self._lib.dmx_coverage_count_resident(self._h, int(handle), int(start), int(stop), int(quality_threshold), ptr(out)))
        return out

    # ---- coverage (include/demux_hip.h: dmx_coverage_count / _candidates / _fetch_candidates; demuxalot_amd/snp_detection.py) ----
    def coverage_count(self, reads, start, stop, quality_threshold=15, fetch=True):
        """int32[4, stop - start] (rows A, C, G, T) counted on the device from a DecodedReads, by the rules of pysam's
        count_coverage; None unless fetched (the window stays on the device for coverage_candidates).  The resident problem stays."""
        desc, _keep_alive = self._reads_descriptor(reads)
        out = np.empty((4, max(0, int(stop) - int(start))), dtype=np.int32) if fetch else None
        check(self._lib.dmx_coverage_count(self._h, desc, int(start), int(stop), int(quality_threshold), ptr(out)))
        return out

    def coverage_candidates(self, minimum_coverage, minimum_alternative_fraction, minimum_alternative_coverage,
                            minimum_fraction_of_ref_and_alt, max_snp_candidates, fetch_counts=False):
        """Candidate positions of the last coverage_count: int32 absolute positions, ascending (with fetch_counts: and their
        int32[n, 4] A, C, G, T counts)."""
        n = ctypes.c_int64(0)
        check(self._lib.dmx_coverage_candidates(self._h, float(minimum_coverage), float(minimum_alternative_fraction),
                                                float(minimum_alternative_coverage), float(minimum_fraction_of_ref_and_alt),
                                                int(max_snp_candidates), ctypes.byref(n)))
        positions = np.empty(n.value, dtype=np.int32)
        counts = np.empty((n.value, 4), dtype=np.int32) if fetch_counts else None
        check(self._lib.dmx_coverage_fetch_candidates(self._h, ptr(positions), ptr(counts)))
        return (positions, counts) if fetch_counts else positions

    def coverage_timings(self):
        """{stage: milliseconds} of the last coverage_count and coverage_candidates (include/demux_hip_debug.h:
        dmx_get_coverage_timings)."""
        ms = (ctypes.c_double * len(_lib.COVERAGE_STAGES))()
        check(self._lib.dmx_get_coverage_timings(self._h, ms))
        return dict(zip(_lib.COVERAGE_STAGES, ms))

    def set_coverage_form(self, form):
        """_lib.COVERAGE_ATOMIC or _lib.COVERAGE_TILED (include/demux_hip_debug.h: dmx_set_coverage_form); same integers."""
        check(self._lib.dmx_set_coverage_form(self._h, int(form)))

    def get_top_options(self, k):
        """The k (<= 4) best options per barcode, best first: (int32[B, k], float32[B, k])."""
        options = np.empty((self.B, int(k)), dtype=np.int32)
        probs = np.empty((self.B, int(k)), dtype=np.float32)
        check(self._lib.dmx_get_top_options(self._h, int(k), ptr(options), ptr(probs)))
        return options, probs

    def get_option_sums(self):
        """probs.sum(axis=0) as float64[K]."""
        out = np.empty(self.K, dtype=np.float64)
        check(self._lib.dmx_get_option_sums(self._h, ptr(out)))
        return out

    def get_donor_readout(self, marginals=False):
        """The pair columns folded back onto donors in one pass (include/demux_hip_debug.h: dmx_get_donor_readout): dict of
        singlet_mass, doublet_mass (float64[B]), best_singlet, best_pair (int32[B] column indices, -1: no such column),
        best_singlet_prob, best_pair_prob (float32[B]) and, with marginals=True, donor_marginals (float32[B, G])."""
        B = self.B
        out = dict(singlet_mass=np.zeros(B, np.float64), doublet_mass=np.zeros(B, np.float64),
                   best_singlet=np.full(B, -1, np.int32), best_singlet_prob=np.full(B, np.nan, np.float32),
                   best_pair=np.full(B, -1, np.int32), best_pair_prob=np.full(B, np.nan, np.float32))
        if marginals:
            out['donor_marginals'] = np.zeros((B, self.G), np.float32)
        check(self._lib.dmx_get_donor_readout(self._h, ptr(out['singlet_mass']), ptr(out['doublet_mass']), ptr(out['best_singlet']),
                                              ptr(out['best_singlet_prob']), ptr(out['best_pair']), ptr(out['best_pair_prob']),
                                              ptr(out.get('donor_marginals'))))
        return out

    def get_allowed_mass(self, start, options):
        """(mass float64[B], best_is_allowed int32[B]) of the CSR lists options[start[b]:start[b + 1]] of allowed option columns:
        the listed posteriors added in float64 in list order, and whether the row's first maximum is listed
        (include/demux_hip_debug.h: dmx_get_allowed_mass)."""
        start, options = as_c(start, np.int64), as_c(options, np.int32)
        assert start.shape == (self.B + 1,), 'one start per barcode and the end'
        assert options.ndim == 1 and len(options) >= (start[-1] if len(start) else 0), 'allowed options shorter than start[-1]'
        mass = np.zeros(self.B, np.float64)
        hit = np.zeros(self.B, np.int32)
        check(self._lib.dmx_get_allowed_mass(self._h, ptr(start), ptr(options), ptr(mass), ptr(hit)))
        return mass, hit

    def _pools_arguments(self, pools, pool_of_barcode, with_doublets, pair_penalty, fetch_logits, fetch_probs):
        """(the pool arguments of the dmx_estep_pools family as ctypes pointers, the arrays behind them, the result dict)."""
        B = self.B
        pool_of_barcode = as_c(pool_of_barcode, np.int32)
        assert pool_of_barcode.shape == (B,), 'one pool id per barcode'
        pair_penalty = as_c(pair_penalty, np.float32)
        assert pair_penalty.shape == (len(pools),), 'one pair penalty per pool'
        pool_start, donors, row_ptr = pooled_layout(pools, pool_of_barcode, with_doublets)
        n = int(row_ptr[-1])
        out = dict(row_ptr=row_ptr, logits=np.empty(n, np.float32) if fetch_logits else None,
                   probs=np.empty(n, np.float32) if fetch_probs else None, best_option=np.full(B, -1, np.int32),
                   best_prob=np.full(B, np.nan, np.float32), doublet_mass=np.full(B, np.nan, np.float64))
        keep = (pool_start, donors, pair_penalty, pool_of_barcode, row_ptr)
        pool_args = (len(pools), ptr(pool_start), ptr(donors), ptr(pair_penalty), ptr(pool_of_barcode), ptr(row_ptr))
        return pool_args, keep, out

    @staticmethod
    def _pools_results(out):
        return (ptr(out['logits']), ptr(out['probs']), ptr(out['best_option']), ptr(out['best_prob']), ptr(out['doublet_mass']))

    def _pooled_call(self, entry, pools, pool_of_barcode, with_doublets, pair_penalty, fetch_logits, fetch_probs, head=(), middle=(),
                     tail=lambda out: (), fetch_addition=None, ambient=False, more=None, dense=False):
        """One call of the dmx_estep_pools family: entry(handle, *head, with_doublets, the pool arguments, *middle, the result
        pointers, *tail(out)) and its result dict.  fetch_addition (not None: an EM entry): the key 'addition', float32[V, G] or None;
        ambient: the key 'ambient', float32[V]; more(n values of a compact matrix): further keys; all there before tail(out) is
        asked.  dense: the entry leaves the dense [B, G] singlet posteriors resident, so K becomes G."""
        pool_args, _keep, out = self._pools_arguments(pools, pool_of_barcode, with_doublets, pair_penalty, fetch_logits, fetch_probs)
        if fetch_addition is not None:
            out['addition'] = np.empty((self.V, self.G), dtype=np.float32) if fetch_addition else None
        if ambient:
            out['ambient'] = np.empty(self.V, np.float32)
        if more is not None:
            out.update(more(int(out['row_ptr'][-1])))
        check(entry(self._h, *head, int(bool(with_doublets)), *pool_args, *middle, *self._pools_results(out), *tail(out)))
        if dense:
            self.K = self.G
        return out

    def estep_pools(self, pools, pool_of_barcode, with_doublets, pair_penalty, fetch_logits=True, fetch_probs=True, resident=False):
        """The pooled E-step (include/demux_hip_debug.h: dmx_estep_pools): every barcode against the donors of its own pool.
        pools: one strictly ascending list of table columns per pool; pool_of_barcode int32[B], -1: in no pool;
        pair_penalty float32[n_pools].  Returns a dict: row_ptr int64[B + 1], logits / probs (compact float32[row_ptr[B]], or
        None), best_option int32[B], best_prob float32[B], doublet_mass float64[B].  The resident results of the last
        E-step are left as they are - unless resident=True (dmx_estep_pools_resident): then the singlet posteriors are left in
        the context as a dense [B, G] matrix, zero outside a barcode's pool, so that mstep() may follow and get_probs() returns it."""
        entry = self._lib.dmx_estep_pools_resident if resident else self._lib.dmx_estep_pools
        return self._pooled_call(entry, pools, pool_of_barcode, with_doublets, pair_penalty, fetch_logits, fetch_probs, dense=resident)

    def em_pools(self, n_iterations, p_genotype_clip, pools, pool_of_barcode, with_doublets, pair_penalty, contribution_power=2.,
                 fetch_logits=True, fetch_probs=True, fetch_addition=True):
        """n_iterations of P-step, pooled E-step and M-step on the device (include/demux_hip_debug.h: dmx_em_pools): em() with every
        barcode scored against the donors of its own pool, and posterior 0 for the others.  Returns estep_pools()'s dict of the last
        iteration with one more key, 'addition': float32[V, G], the addition its E-step used (None without fetch_addition).
        get_learnt_betas() and get_probs() (the dense [B, G] singlet posteriors) work afterwards."""
        return self._pooled_call(self._lib.dmx_em_pools, pools, pool_of_barcode, with_doublets, pair_penalty, fetch_logits, fetch_probs,
                                 head=(int(n_iterations), *self.clip_bounds(p_genotype_clip)), middle=(float(contribution_power),),
                                 tail=lambda out: (ptr(out['addition']),), fetch_addition=bool(fetch_addition), dense=True)

    def ambient_profile(self, donor1, donor2, alphas, p_genotype_clip=0.01, ambient=None, fetch_profile=True):
        """Ambient RNA fractions (include/demux_hip_debug.h: dmx_ambient_profile): the log-likelihood of every barcode's calls under
        its assigned option mixed with the soup's allele profile, on the grid `alphas` (float32, 1 .. 64 values in [0, 1]).
        donor1 / donor2: int32[B] table columns as donor_readout.column_donors gives them ((-1, .) skipped, (d, -1) a singlet, d1 < d2 a
        pair); ambient: float32[V] or None (derived from the resident calls, clipped as the genotype table is).  Returns a dict:
        loglik float32[B, A] (None without fetch_profile), best int32[B], ll_best, ll_zero float32[B], ambient float32[V] (the profile
        that was used).  The resident results of the last E-step are left as they are."""
        B = self.B
        alphas = as_c(alphas, np.float32)
        assert alphas.ndim == 1, 'the grid is one-dimensional'
        donor1, donor2 = as_c(donor1, np.int32), as_c(donor2, np.int32)
        assert donor1.shape == (B,) and donor2.shape == (B,), 'one option per barcode'
        ambient = self._ambient_argument(ambient)
        lo, hi = self.clip_bounds(p_genotype_clip)
        A = len(alphas)
        out = dict(loglik=np.empty((B, A), np.float32) if fetch_profile else None, best=np.full(B, -1, np.int32),
                   ll_best=np.full(B, np.nan, np.float32), ll_zero=np.full(B, np.nan, np.float32), ambient=np.empty(self.V, np.float32))
        check(self._lib.dmx_ambient_profile(self._h, lo, hi, A, ptr(alphas), ptr(donor1), ptr(donor2), ptr(ambient), ptr(out['loglik']),
                                            ptr(out['best']), ptr(out['ll_best']), ptr(out['ll_zero']), ptr(out['ambient'])))
        return out

    def estep_ambient(self, pools, pool_of_barcode, with_doublets, pair_penalty, alpha, p_genotype_clip=0.01, ambient=None,
                      fetch_logits=True, fetch_probs=True, resident=False):
        """The pooled E-step under per-barcode ambient fractions (include/demux_hip_debug.h: dmx_estep_ambient): estep_pools() with
        every option scored as q (1 - alpha[b]) + ambient[v] alpha[b].  alpha: float32[B] in [0, 1] (not looked at for a barcode in no
        pool); ambient: float32[V] or None (derived from the resident calls, clipped as the genotype table is).  Returns
        estep_pools()'s dict with one more key, 'ambient': float32[V], the profile that was used.  The resident results of the last
        E-step are left as they are - unless resident=True (dmx_estep_ambient_resident): then the singlet posteriors are left in the
        context as a dense [B, G] matrix, zero outside a barcode's pool, so that mstep_ambient() or mstep() may follow and get_probs()
        returns it."""
        alpha, ambient = self._ambient_arguments(alpha, ambient)
        lo, hi = self.clip_bounds(p_genotype_clip)
        entry = self._lib.dmx_estep_ambient_resident if resident else self._lib.dmx_estep_ambient
        return self._pooled_call(entry, pools, pool_of_barcode, with_doublets, pair_penalty, fetch_logits, fetch_probs, ambient=True,
                                 tail=lambda out: (lo, hi, ptr(alpha), ptr(ambient), ptr(out['ambient'])), dense=resident)

    def _ambient_argument(self, ambient):
        """The soup's profile as every entry under ambient fractions takes it: float32[V], or None (derived from the resident calls)."""
        if ambient is not None:
            ambient = as_c(ambient, np.float32)
            assert ambient.shape == (self.V,), 'one ambient value per variant'
        return ambient

    def _ambient_arguments(self, alpha, ambient):
        """(alpha float32[B], ambient float32[V] or None) as the entries under per-barcode fractions take them."""
        alpha = as_c(alpha, np.float32)
        assert alpha.shape == (self.B,), 'one fraction per barcode'
        return alpha, self._ambient_argument(ambient)

    def mstep_ambient(self, alpha, contribution_power=2., p_genotype_clip=0.01, ambient=None, fetch=True):
        """The M-step under per-barcode ambient fractions (include/demux_hip_debug.h: dmx_mstep_ambient): mstep() with every call's
        contribution weighted by the probability that the call came from the donor and not from the soup,
        r = own / (own + ambient[v] alpha[b]), own = genotype_prob[v, g] (1 - alpha[b]), on the resident posteriors and the table of
        the last P-step.  alpha: float32[B] in [0, 1], every barcode's is read; ambient: float32[V] or None (derived from the resident
        calls, clipped as the genotype table is).  The sums are float64 in the reference's order whatever the E-step mode.  Returns
        the addition float32[V, G] (None without fetch); it becomes the context's, as after mstep()."""
        alpha, ambient = self._ambient_arguments(alpha, ambient)
        lo, hi = self.clip_bounds(p_genotype_clip)
        addition = np.empty((self.V, self.G), dtype=np.float32) if fetch else None
        check(self._lib.dmx_mstep_ambient(self._h, float(contribution_power), ptr(alpha), ptr(ambient), lo, hi, ptr(addition)))
        return addition

    def em_ambient(self, n_iterations, p_genotype_clip, pools, pool_of_barcode, with_doublets, pair_penalty, alpha, ambient=None,
                   contribution_power=2., fetch_logits=True, fetch_probs=True, fetch_addition=True):
        """n_iterations of P-step, dense E-step under the fractions and weighted M-step on the device (include/demux_hip_debug.h:
        dmx_em_ambient): em_pools() with estep_ambient() and mstep_ambient() in place of its two steps; the soup's profile is fixed for
        the call.  Returns em_pools()'s dict with one more key, 'ambient': float32[V], the profile that was used.  get_learnt_betas()
        and get_probs() (the dense [B, G] singlet posteriors) work afterwards."""
        alpha, ambient = self._ambient_arguments(alpha, ambient)
        return self._pooled_call(self._lib.dmx_em_ambient, pools, pool_of_barcode, with_doublets, pair_penalty, fetch_logits, fetch_probs,
                                 head=(int(n_iterations), *self.clip_bounds(p_genotype_clip)),
                                 middle=(float(contribution_power), ptr(alpha), ptr(ambient)),
                                 tail=lambda out: (ptr(out['addition']), ptr(out['ambient'])), fetch_addition=bool(fetch_addition),
                                 ambient=True, dense=True)

    def mstep_soup(self, alpha, pseudo_count=1., p_genotype_clip=0.01, ambient=None):
        """The M-step of the soup's allele profile (include/demux_hip_debug.h: dmx_mstep_soup): every call counts for the soup with
        the probability that it came from there, s = amb / (own + amb), amb = ambient[v] alpha[b], own = genotype_prob[v, g]
        (1 - alpha[b]), on the resident posteriors and the table of the last P-step.  alpha: float32[B] in [0, 1], every barcode's is
        read; ambient: float32[V] or None - the profile the posteriors were scored with (None: the derived one).  Returns
        (ambient' float32[V], counts float32[V]): the new profile - the P-step's formula on counts + pseudo_count, clipped - and the
        soup's expected calls per variant.  The context's addition, posteriors and table stay as they are."""
        alpha, ambient = self._ambient_arguments(alpha, ambient)
        lo, hi = self.clip_bounds(p_genotype_clip)
        profile, counts = np.empty(self.V, np.float32), np.empty(self.V, np.float32)
        check(self._lib.dmx_mstep_soup(self._h, ptr(alpha), ptr(ambient), float(pseudo_count), lo, hi, ptr(profile), ptr(counts)))
        return profile, counts

    def em_ambient_soup(self, n_iterations, p_genotype_clip, pools, pool_of_barcode, with_doublets, pair_penalty, alpha, ambient=None,
                        pseudo_count=1., contribution_power=2., fetch_logits=True, fetch_probs=True, fetch_addition=True):
        """em_ambient() with the soup's profile learnt (include/demux_hip_debug.h: dmx_em_ambient_soup): behind every E-step but the
        last, mstep_soup() and mstep_ambient(), both with the profile that E-step read; the new profile takes effect in the next
        iteration.  ambient: the first iteration's profile (None: the derived one).  Returns em_ambient()'s dict - 'ambient' is the
        profile the LAST E-step read - with one more key, 'counts': float32[V], the totals that profile was formed from (zeros with
        one iteration)."""
        alpha, ambient = self._ambient_arguments(alpha, ambient)
        return self._pooled_call(self._lib.dmx_em_ambient_soup, pools, pool_of_barcode, with_doublets, pair_penalty, fetch_logits, fetch_probs,
                                 head=(int(n_iterations), *self.clip_bounds(p_genotype_clip)),
                                 middle=(float(contribution_power), ptr(alpha), ptr(ambient), float(pseudo_count)),
                                 tail=lambda out: (ptr(out['addition']), ptr(out['ambient']), ptr(out['counts'])),
                                 fetch_addition=bool(fetch_addition), ambient=True, more=lambda _n: dict(counts=np.empty(self.V, np.float32)),
                                 dense=True)

    def em_doublets(self, n_iterations, p_genotype_clip, pools, pool_of_barcode, with_doublets, pair_penalty, min_pair_posterior=1e-3,
                    contribution_power=2., fetch_logits=True, fetch_probs=True, fetch_addition=True):
        """n_iterations of P-step, dense pooled E-step and the M-step that also learns from doublet posteriors, on the device
        (include/demux_hip_debug.h: dmx_em_doublets): em_pools() whose M-step credits each donor of a pair option at or above
        min_pair_posterior with its share of every call, r = own / (own + other), weighted by the pair's posterior.  The sums are
        float64 in the reference's order whatever the E-step mode.  Returns em_pools()'s dict.  get_learnt_betas() and get_probs()
        (the dense [B, G] singlet posteriors) work afterwards."""
        return self._pooled_call(self._lib.dmx_em_doublets, pools, pool_of_barcode, with_doublets, pair_penalty, fetch_logits, fetch_probs,
                                 head=(int(n_iterations), *self.clip_bounds(p_genotype_clip)),
                                 middle=(float(contribution_power), float(min_pair_posterior)),
                                 tail=lambda out: (ptr(out['addition']),), fetch_addition=bool(fetch_addition), dense=True)

    def mstep_doublets(self, pools, pool_of_barcode, with_doublets, pair_penalty, post_rows, min_pair_posterior=1e-3, contribution_power=2.,
                       fetch=True):
        """The M-step that also learns from doublet posteriors (include/demux_hip_debug.h: dmx_mstep_doublets) on the resident dense
        posteriors and the table of the last P-step: post_rows is the compact 'probs' estep_pools(..., resident=True) returned for
        the same pools.  Returns the addition float32[V, G] (None without fetch); it becomes the context's, as after mstep()."""
        pool_args, _keep, out = self._pools_arguments(pools, pool_of_barcode, with_doublets, pair_penalty, False, False)
        post_rows = as_c(post_rows, np.float32)
        assert post_rows.ndim == 1, 'the compact rows are one-dimensional'
        addition = np.empty((self.V, self.G), dtype=np.float32) if fetch else None
        check(self._lib.dmx_mstep_doublets(self._h, float(contribution_power), float(min_pair_posterior), int(bool(with_doublets)), *pool_args,
                                           ptr(post_rows), len(post_rows), ptr(addition)))
        return addition

    def estep_ambient_grid(self, pools, pool_of_barcode, with_doublets, pair_penalty, alphas, p_genotype_clip=0.01, ambient=None,
                           fetch_logits=True, fetch_probs=True, fetch_alpha_index=True, fetch_profile=False, over_grid='max', log_weights=None,
                           fetch_alpha_mean=True):
        """The pooled E-step with every option at its own best ambient fraction (include/demux_hip_debug.h: dmx_estep_ambient_grid):
        estep_ambient() on the grid `alphas` (float32, 1 .. 64 values in [0, 1], any order), every option's logit its first maximum
        over the grid, one softmax over those.  ambient: float32[V] or None (derived from the resident calls, clipped as the genotype
        table is).  Returns estep_pools()'s dict with more keys: 'ambient' float32[V], the profile that was used; 'alphas', the grid;
        'alpha_index' int32[row_ptr[B]], the grid point of every option's maximum (None without fetch_alpha_index);
        'best_alpha_index' int32[B], that of best_option (-1: none); 'profile' float32[row_ptr[B], A], every option's logit at every
        grid point (None without fetch_profile: A times the logits' memory).  The resident results of the last E-step are left as
        they are.
        over_grid='marginal' (dmx_estep_ambient_grid_marginal): every option's logit is the log of the sum over the grid of
        exp(its logit there + log_weights) instead of the maximum; log_weights: float32[A], the log of a prior over the grid, or None
        (all 0).  'alpha_index' is then the first maximum of logit + log_weights, and there are two more keys: 'alpha_mean'
        float32[row_ptr[B]], every option's posterior mean fraction (None without fetch_alpha_mean), 'best_alpha_mean' float32[B],
        that of best_option (NaN: none).  The profile is the max mode's: fetch_profile with 'marginal' raises."""
        if over_grid not in ('max', 'marginal'):
            raise ValueError(f"over_grid is 'max' or 'marginal', not {over_grid!r}")
        marginal = over_grid == 'marginal'
        if marginal and fetch_profile:
            raise ValueError("the profile is not kept with over_grid='marginal': ask for it with over_grid='max'")
        if log_weights is not None and not marginal:
            raise ValueError("log_weights are the prior of over_grid='marginal'; the maximum takes none")
        alphas = as_c(alphas, np.float32)
        assert alphas.ndim == 1, 'the grid is one-dimensional'
        if log_weights is not None:
            log_weights = as_c(log_weights, np.float32)
            assert log_weights.shape == alphas.shape, 'one log weight per grid value'
        ambient = self._ambient_argument(ambient)
        lo, hi = self.clip_bounds(p_genotype_clip)
        A = len(alphas)

        def more(n):
            keys = dict(alphas=alphas, alpha_index=np.full(n, -1, np.int32) if fetch_alpha_index else None,
                        best_alpha_index=np.full(self.B, -1, np.int32), profile=np.empty((n, A), np.float32) if fetch_profile else None)
            if marginal:
                keys.update(alpha_mean=np.full(n, np.nan, np.float32) if fetch_alpha_mean else None,
                            best_alpha_mean=np.full(self.B, np.nan, np.float32))
            return keys

        def tail(out):
            grid = (lo, hi, A, ptr(alphas), ptr(ambient), ptr(out['ambient']), ptr(out['alpha_index']), ptr(out['best_alpha_index']))
            if marginal:
                return (*grid, ptr(log_weights), ptr(out['alpha_mean']), ptr(out['best_alpha_mean']))
            return (*grid, ptr(out['profile']))

        entry = self._lib.dmx_estep_ambient_grid_marginal if marginal else self._lib.dmx_estep_ambient_grid
        return self._pooled_call(entry, pools, pool_of_barcode, with_doublets, pair_penalty, fetch_logits, fetch_probs, ambient=True, more=more,
                                 tail=tail)

    def _shares_arguments(self, shares, log_weights):
        """(shares float32[n], log_weights float32[n] or None) as the entries over a grid of mixing shares take them."""
        shares = as_c(shares, np.float32)
        assert shares.ndim == 1, 'the grid is one-dimensional'
        if log_weights is not None:
            log_weights = as_c(log_weights, np.float32)
            assert log_weights.shape == shares.shape, 'one log weight per share'
        return shares, log_weights

    def _shares_results(self, shares, fetch_share_index, fetch_share_mean):
        """more(n) of _pooled_call for the share outputs, and the pointers to them in the entries' order."""
        def more(n):
            return dict(shares=shares, share_index=np.full(n, -1, np.int32) if fetch_share_index else None,
                        share_mean=np.full(n, np.nan, np.float32) if fetch_share_mean else None,
                        best_share_index=np.full(self.B, -1, np.int32), best_share_mean=np.full(self.B, np.nan, np.float32))

        def pointers(out):
            return (ptr(out['share_index']), ptr(out['share_mean']), ptr(out['best_share_index']), ptr(out['best_share_mean']))

        return more, pointers

    def em_doublet_shares(self, n_iterations, p_genotype_clip, pools, pool_of_barcode, with_doublets, pair_penalty, shares, log_weights=None,
                          min_pair_posterior=1e-3, contribution_power=2., fetch_logits=True, fetch_probs=True, fetch_addition=True,
                          fetch_share_index=True, fetch_share_mean=True):
        """n_iterations of P-step, the dense E-step over a grid of mixing shares and the M-step that credits a live pair's donors at
        the pair's posterior mean share, on the device (include/demux_hip_debug.h: dmx_em_doublet_shares): em_doublets() with
        estep_pair_shares() as its E-step and r = own w_own / (own w_own + other w_other) as a donor's responsibility.  Returns
        em_doublets()'s dict with estep_pair_shares()'s share keys of the last E-step.  get_learnt_betas() and get_probs() (the dense
        [B, G] singlet posteriors) work afterwards."""
        shares, log_weights = self._shares_arguments(shares, log_weights)
        more, pointers = self._shares_results(shares, fetch_share_index, fetch_share_mean)
        return self._pooled_call(self._lib.dmx_em_doublet_shares, pools, pool_of_barcode, with_doublets, pair_penalty, fetch_logits, fetch_probs,
                                 head=(int(n_iterations), *self.clip_bounds(p_genotype_clip)),
                                 middle=(float(contribution_power), float(min_pair_posterior), len(shares), ptr(shares), ptr(log_weights)),
                                 tail=lambda out: (ptr(out['addition']), *pointers(out)), fetch_addition=bool(fetch_addition), more=more,
                                 dense=True)

    def mstep_doublet_shares(self, pools, pool_of_barcode, with_doublets, pair_penalty, post_rows, share_rows, min_pair_posterior=1e-3,
                             contribution_power=2., fetch=True):
        """The M-step that learns from doublets of unequal shares (include/demux_hip_debug.h: dmx_mstep_doublet_shares) on the resident
        dense posteriors and the table of the last P-step: post_rows and share_rows are the compact 'probs' and 'share_mean'
        estep_pair_shares(..., resident=True) returned for the same pools.  Returns the addition float32[V, G] (None without fetch);
        it becomes the context's, as after mstep()."""
        pool_args, _keep, out = self._pools_arguments(pools, pool_of_barcode, with_doublets, pair_penalty, False, False)
        post_rows = as_c(post_rows, np.float32)
        assert post_rows.ndim == 1, 'the compact rows are one-dimensional'
        if share_rows is not None:
            share_rows = as_c(share_rows, np.float32)
            assert share_rows.shape == post_rows.shape, 'one share per posterior of the rows'
        addition = np.empty((self.V, self.G), dtype=np.float32) if fetch else None
        check(self._lib.dmx_mstep_doublet_shares(self._h, float(contribution_power), float(min_pair_posterior), int(bool(with_doublets)),
                                                 *pool_args, ptr(post_rows), ptr(share_rows), len(post_rows), ptr(addition)))
        return addition

    def estep_pair_shares(self, pools, pool_of_barcode, with_doublets, pair_penalty, shares, log_weights=None, fetch_logits=True,
                          fetch_probs=True, fetch_share_index=True, fetch_share_mean=True, resident=False):
        """The pooled E-step with every pair option summed over a grid of mixing shares (include/demux_hip_debug.h:
        dmx_estep_pair_shares): estep_pools() with a pair (d1, d2) scored as prob[d1] w + prob[d2] (1 - w) at every w of `shares`
        (float32, 1 .. 64 values in [0, 1], any order) and its logit the log of the sum over the grid of exp(its logit there +
        log_weights); singlet options are estep_pools()'s own.  log_weights: float32[n_shares], the log of a prior over the grid, or
        None (all 0: the log of a plain sum, not of a mean).  Returns estep_pools()'s dict with more keys: 'shares', the grid;
        'share_index' int32[row_ptr[B]], the grid point of every pair's largest term (-1: a singlet; None without fetch_share_index);
        'share_mean' float32[row_ptr[B]], every pair's posterior mean share of its first donor (NaN: a singlet; None without
        fetch_share_mean); 'best_share_index' int32[B] and 'best_share_mean' float32[B], those of best_option (-1 / NaN: a singlet
        or none).  The resident results of the last E-step are left as they are - unless resident=True
        (dmx_estep_pair_shares_resident): then the singlet posteriors are left in the context as a dense [B, G] matrix, zero outside a
        barcode's pool, so that mstep_doublet_shares() or mstep() may follow and get_probs() returns it."""
        shares, log_weights = self._shares_arguments(shares, log_weights)
        more, pointers = self._shares_results(shares, fetch_share_index, fetch_share_mean)
        entry = self._lib.dmx_estep_pair_shares_resident if resident else self._lib.dmx_estep_pair_shares
        return self._pooled_call(entry, pools, pool_of_barcode, with_doublets, pair_penalty, fetch_logits, fetch_probs, more=more,
                                 tail=lambda out: (len(shares), ptr(shares), ptr(log_weights), *pointers(out)), dense=resident)

    # ---- pooled results kept resident (include/demux_hip_debug.h "Pooled results kept resident"; csrc/pooled_readout.hip) ----
    def set_keep_pooled(self, keep):
        """With True, estep_pools(), estep_ambient() and estep_ambient_grid() (not their resident / EM siblings) leave their compact
        result in the context's pooled slot (dmx_set_keep_pooled)."""
        check(self._lib.dmx_set_keep_pooled(self._h, int(bool(keep))))

    def pooled_upload(self, n_donors, pools, pool_of_barcode, with_doublets, probs, logits=None):
        """Fills the pooled slot from host arrays (dmx_pooled_upload): pools as estep_pools() takes them (columns below n_donors),
        pool_of_barcode int32[B], compact float32 probs (and logits, or None).  Returns row_ptr int64[B + 1]."""
        pool_of_barcode = as_c(pool_of_barcode, np.int32)
        pool_start, donors, row_ptr = pooled_layout(pools, pool_of_barcode, with_doublets)
        probs = as_c(probs, np.float32)
        assert probs.shape == (int(row_ptr[-1]),), 'compact probs: row_ptr[B] values'
        if logits is not None:
            logits = as_c(logits, np.float32)
            assert logits.shape == probs.shape, 'compact logits: row_ptr[B] values'
        check(self._lib.dmx_pooled_upload(self._h, len(pool_of_barcode), int(n_donors), int(bool(with_doublets)), len(pools), ptr(pool_start),
                                          ptr(donors), ptr(pool_of_barcode), ptr(row_ptr), ptr(logits), ptr(probs)))
        return row_ptr

    def pooled_info(self):
        """dict of _lib.POOLED_INFO (dmx_pooled_info): present, B, n_pools, n_values, with_doublets, has_logits, has_alpha_index,
        has_alpha_mean."""
        info = (ctypes.c_int64 * len(_lib.POOLED_INFO))()
        check(self._lib.dmx_pooled_info(self._h, info))
        return dict(zip(_lib.POOLED_INFO, (int(v) for v in info)))

    def pooled_release(self):
        check(self._lib.dmx_pooled_release(self._h))

    def pooled_get(self, what, b0, b1, n_values):
        """The compact entries of barcodes [b0, b1) of 'logits' | 'probs' | 'alpha_index' | 'alpha_mean' (dmx_pooled_get); n_values:
        row_ptr[b1] - row_ptr[b0], which the caller knows."""
        code, dtype = _lib.POOLED_WHAT[what]
        out = np.empty(int(n_values), dtype=dtype)
        check(self._lib.dmx_pooled_get(self._h, code, int(b0), int(b1), ptr(out)))
        return out

    def pooled_get_pool(self, what, pool, n_barcodes, n_options):
        """[n_barcodes, n_options] rows of one pool's barcodes, ascending (dmx_pooled_get_pool)."""
        code, dtype = _lib.POOLED_WHAT[what]
        out = np.empty((int(n_barcodes), int(n_options)), dtype=dtype)
        check(self._lib.dmx_pooled_get_pool(self._h, code, int(pool), ptr(out)))
        return out

    def _pooled_staging(self, name, shape, dtype):
        """A download target of the pooled read-outs that outlives the call.  The runtime pins the pages of a pageable download's
        target; giving fresh arrays back to the allocator after every call made the next calls wait 10 - 30 ms each at 200 000
        barcodes (scripts/pooled_readout_timing.py), where the same call into arrays that stay takes 0.7 ms.  The read-outs
        therefore land here and the caller gets copies."""
        buffers = self.__dict__.setdefault('_pooled_buffers', {})
        held = buffers.get(name)
        if held is None or held.shape != tuple(np.atleast_1d(shape)) or held.dtype != np.dtype(dtype):
            held = buffers[name] = np.zeros(shape, dtype)
        return held

    def pooled_readout(self, marginals=False, masses=True):
        """One pass over the slot's posteriors (dmx_pooled_readout): dict of singlet_mass, doublet_mass (float64[B]; None without
        masses), best_option, best_singlet, best_pair (int32[B], pool-local, -1: none) with best_prob, best_singlet_prob,
        best_pair_prob (float32[B]) and, with marginals=True, marg_ptr (int64[B + 1]) and donor_marginals (compact float32)."""
        B = self.pooled_info()['B']
        kinds = dict(singlet_mass=np.float64, doublet_mass=np.float64, best_option=np.int32, best_prob=np.float32, best_singlet=np.int32,
                     best_singlet_prob=np.float32, best_pair=np.int32, best_pair_prob=np.float32)
        stage = {name: None if not masses and name.endswith('_mass') else self._pooled_staging(name, B, kind) for name, kind in kinds.items()}
        marg_ptr = marg = None
        if marginals:
            marg_ptr = np.empty(B + 1, np.int64)
            check(self._lib.dmx_pooled_readout(self._h, *([None] * len(kinds)), ptr(marg_ptr), None))  # (sizes only: nothing is launched for them)
            marg = self._pooled_staging('donor_marginals', int(marg_ptr[-1]), np.float32)
        check(self._lib.dmx_pooled_readout(self._h, *(ptr(stage[name]) for name in kinds), None, ptr(marg)))
        out = {name: None if held is None else held.copy() for name, held in stage.items()}
        if marginals:
            out['marg_ptr'], out['donor_marginals'] = marg_ptr, marg.copy()
        return out

    def pooled_top_options(self, k):
        """(int32[B, k] pool-local options, float32[B, k]), best first (dmx_pooled_top_options)."""
        B = self.pooled_info()['B']
        options, probs = self._pooled_staging('top_options', (B, int(k)), np.int32), self._pooled_staging('top_probs', (B, int(k)), np.float32)
        check(self._lib.dmx_pooled_top_options(self._h, int(k), ptr(options), ptr(probs)))
        return options.copy(), probs.copy()

    def pooled_option_sums(self, n_options_total):
        """(float64[n_options_total] option sums, pool after pool; int64[n_pools] barcodes per pool) - dmx_pooled_option_sums."""
        sums = np.zeros(int(n_options_total), np.float64)
        counts = np.zeros(self.pooled_info()['n_pools'], np.int64)
        check(self._lib.dmx_pooled_option_sums(self._h, ptr(sums), ptr(counts)))
        return sums, counts

    def pooled_allowed_mass(self, start, options):
        """get_allowed_mass() on the slot, with pool-local options (dmx_pooled_allowed_mass)."""
        B = self.pooled_info()['B']
        start, options = as_c(start, np.int64), as_c(options, np.int32)
        assert start.shape == (B + 1,), 'one start per barcode and the end'
        assert options.ndim == 1 and len(options) >= (start[-1] if len(start) else 0), 'allowed options shorter than start[-1]'
        mass, hit = self._pooled_staging('allowed_mass', B, np.float64), self._pooled_staging('allowed_hit', B, np.int32)
        check(self._lib.dmx_pooled_allowed_mass(self._h, ptr(start), ptr(options), ptr(mass), ptr(hit)))
        return mass.copy(), hit.copy()

    def synchronize(self):
        check(self._lib.dmx_synchronize(self._h))

    # ---- multi-GPU ----------------------------------------------------------------------
    @staticmethod
    def new_unique_id() -> bytes:
        buf = ctypes.create_string_buffer(_lib.UNIQUE_ID_BYTES)
        check(_lib.load().dmx_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, rank, nranks, unique_id: bytes, reduce_dtype='f64'):
        assert len(unique_id) == _lib.UNIQUE_ID_BYTES
        buf = ctypes.create_string_buffer(unique_id, _lib.UNIQUE_ID_BYTES)
        check(self._lib.dmx_comm_init(self._h, int(rank), int(nranks), buf, DMX_F64 if reduce_dtype == 'f64' else DMX_F32))

    def comm_init_host(self, rank, nranks, collective, reduce_dtype='f64'):
        """The exchange over the caller's collectives instead of RCCL (include/demux_hip.h: dmx_comm_init_host).
        collective(op, array): op in ('all_reduce', 'reduce_scatter', 'all_gather'); array is the host buffer as a
        numpy view, float32 or float64 - [count] for all_reduce (sum in place), [nranks, count] otherwise
        (reduce_scatter: row `rank` must hold the sum over ranks of their row `rank`; all_gather: row `rank` is
        filled, every row must be on return).  An exception fails the calling step."""
        names = {_lib.COLL_ALL_REDUCE: 'all_reduce', _lib.COLL_REDUCE_SCATTER: 'reduce_scatter', _lib.COLL_ALL_GATHER: 'all_gather'}

        def trampoline(_user, op, buf, count, dtype):
            try:
                kind = np.float64 if dtype == DMX_F64 else np.float32
                n = count if op == _lib.COLL_ALL_REDUCE else count * nranks
                raw = (ctypes.c_char * (n * np.dtype(kind).itemsize)).from_address(buf)
                view = np.frombuffer(raw, dtype=kind)
                collective(names[op], view if op == _lib.COLL_ALL_REDUCE else view.reshape(nranks, count))
                return 0
            except Exception:  # noqa: BLE001 - the C side turns the code into DemuxHipError
                import traceback
                traceback.print_exc()
                return 1
        self._host_collective = _lib.HOST_COLLECTIVE(trampoline)  # kept alive with the context
        check(self._lib.dmx_comm_init_host(self._h, int(rank), int(nranks), self._host_collective, None,
                                           DMX_F64 if reduce_dtype == 'f64' else DMX_F32))

    def comm_init_emulated(self, rank, nranks, link_gbytes_per_s=50.0, latency_us=10.0, reduce_dtype='f64'):
        """This context as rank `rank` of `nranks` over an EMULATED wire (include/demux_hip.h: dmx_comm_init_emulated): for
        timing the exchange schedule on one GPU; the results of such a run are not an EM of any experiment."""
        check(self._lib.dmx_comm_init_emulated(self._h, int(rank), int(nranks), float(link_gbytes_per_s), float(latency_us),
                                               DMX_F64 if reduce_dtype == 'f64' else DMX_F32))

    def exchange_compact(self):
        """(E-steps whose posterior rows travelled as a list, E-steps that fell back to the whole table, rows a list can hold; 0: the
        compact form is off) - include/demux_hip_debug.h: dmx_get_exchange_compact."""
        taken, overflows, cap = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        check(self._lib.dmx_get_exchange_compact(self._h, ctypes.byref(taken), ctypes.byref(overflows), ctypes.byref(cap)))
        return int(taken.value), int(overflows.value), int(cap.value)

    def exchange_compact_table(self):
        """The same for the all-gather of genotype_prob behind the sliced P-step (dmx_get_exchange_compact_table)."""
        taken, overflows, cap = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        check(self._lib.dmx_get_exchange_compact_table(self._h, ctypes.byref(taken), ctypes.byref(overflows), ctypes.byref(cap)))
        return int(taken.value), int(overflows.value), int(cap.value)

    def exchange_mode(self):
        """None (no communicator) | 'variant' (M-step sharded on variants, posteriors all-gathered) | 'reduce_scatter' |
        'allreduce' (exchanges of the per-rank sums); include/demux_hip_debug.h: dmx_get_exchange_mode."""
        mode = ctypes.c_int32(0)
        check(self._lib.dmx_get_exchange_mode(self._h, ctypes.byref(mode)))
        return {0: None, 1: 'variant', 2: 'reduce_scatter', 3: 'allreduce'}[mode.value]

    def set_estep_mode(self, mode):
        """'exact' (logits / posteriors bit-identical to the reference), 'guarded' (tolerance-mode arithmetic, every
        barcode whose posteriors are not provably within the contract's 1e-5 of the reference's - or whose argmax could
        differ - redone exactly) or 'fast' (tolerance mode, unguarded); include/demux_hip.h: dmx_set_estep_mode."""
        check(self._lib.dmx_set_estep_mode(self._h, {'exact': 0, 'fast': 1, 'guarded': 2}[mode]))

    def guard_stats(self):
        """(barcodes the last guarded E-step redid exactly, the same over all E-steps since reset_timings, barcode rows
        those E-steps walked); include/demux_hip_debug.h: dmx_get_guard_stats."""
        last, total, rows = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        check(self._lib.dmx_get_guard_stats(self._h, ctypes.byref(last), ctypes.byref(total), ctypes.byref(rows)))
        return last.value, total.value, rows.value

    def set_guard_adaptive(self, adaptive):
        """Guarded mode: the passes are timed on the device and every E-step takes the cheapest of coarse pass + redo, fine pass + redo
        and the exact kernel on every barcode (default on; off: never the last one; include/demux_hip.h: dmx_set_guard_adaptive)."""
        check(self._lib.dmx_set_guard_adaptive(self._h, int(bool(adaptive))))

    def set_coarse_pass(self, coarse):
        """Guarded mode: E-steps whose logits nobody reads may take the coarse pass (binary16 genotype table; default on;
        'always': every E-step, single ones included - their logits then carry the coarse bound; include/demux_hip.h: dmx_set_coarse_pass)."""
        check(self._lib.dmx_set_coarse_pass(self._h, 2 if coarse == 'always' else int(bool(coarse))))

    def set_lean_memory(self, lean):
        """Memory before speed for the E-steps whose logits are kept: the tile-major copy of the E-step records (16 of 67 bytes per call) is
        released once the coarse pass's records are built from it (include/demux_hip.h: dmx_set_lean_memory; default off)."""
        check(self._lib.dmx_set_lean_memory(self._h, int(bool(lean))))

    def set_mstep_incremental(self, incremental):
        """Default mode, tile-major M-step: update the kept integer sums for the barcodes whose posteriors changed instead of summing every
        call again (same bits; default on; include/demux_hip.h: dmx_set_mstep_incremental)."""
        check(self._lib.dmx_set_mstep_incremental(self._h, 2 if incremental == 'bootstrap' else int(bool(incremental))))

    def mstep_incremental(self):
        """(full passes, delta passes since reset_timings, barcodes the last delta pass visited)"""
        full, delta, last = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        check(self._lib.dmx_get_mstep_incremental(self._h, ctypes.byref(full), ctypes.byref(delta), ctypes.byref(last)))
        return full.value, delta.value, last.value

    def guard_levels(self):
        """dict: level of the last guarded E-step (0 coarse, 1 fine, 2 direct, -1 none), coarse E-steps since reset_timings, barcodes
        flagged by the fine / coarse guard in the last one, the device's timings of the passes in ms (dmx_get_guard_levels)."""
        level = ctypes.c_int32()
        steps, fine, coarse = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        c_ms, f_ms, e_ms = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        check(self._lib.dmx_get_guard_levels(self._h, ctypes.byref(level), ctypes.byref(steps), ctypes.byref(fine), ctypes.byref(coarse),
                                             ctypes.byref(c_ms), ctypes.byref(f_ms), ctypes.byref(e_ms)))
        return {'level': level.value, 'coarse_steps': steps.value, 'flagged_fine': fine.value, 'flagged_coarse': coarse.value,
                'coarse_pass_ms': c_ms.value, 'fine_pass_ms': f_ms.value, 'exact_pass_ms': e_ms.value}

    def set_logits_needed(self, needed):
        """False: nobody will read the logits of the last E-step of the em / run_iterations calls that follow (learn_genotypes returns
        posteriors only), so that E-step too may take the coarse pass; get_logits / get_block('logits') then raise until an E-step
        keeps its logits again (include/demux_hip.h: dmx_set_logits_needed).  Default True."""
        check(self._lib.dmx_set_logits_needed(self._h, int(bool(needed))))

    def guard_probes(self):
        """(E-steps that ran another level than the cheapest to have it timed again since reset_timings, E-steps in a row on the
        current level); include/demux_hip.h: dmx_get_guard_probes."""
        probes, streak = ctypes.c_int64(), ctypes.c_int64()
        check(self._lib.dmx_get_guard_probes(self._h, ctypes.byref(probes), ctypes.byref(streak)))
        return probes.value, streak.value

    def debug_set_pass_ms(self, coarse=-1.0, fine=-1.0, exact=-1.0):
        """Testing aid: overwrite the device's own times of the passes (include/demux_hip.h: dmx_debug_set_pass_ms)."""
        check(self._lib.dmx_debug_set_pass_ms(self._h, float(coarse), float(fine), float(exact)))

    def guard_direct(self):
        """(the last guarded E-step ran direct, E-steps run direct since reset_timings, barcodes the last one queued or -
        direct - would have queued); include/demux_hip.h: dmx_get_guard_direct."""
        return self.guard_state()[:3]

    def guard_state(self):
        """guard_direct() + the device's own timings of the two passes: (..., fast pass over all barcodes in ms, exact kernel
        over all barcodes in ms; 0 = not known yet, negative = estimated from the redo's share, not yet measured)."""
        last, steps, would = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0)
        fast_ms, exact_ms = ctypes.c_double(0), ctypes.c_double(0)
        check(self._lib.dmx_get_guard_direct(self._h, ctypes.byref(last), ctypes.byref(steps), ctypes.byref(would),
                                             ctypes.byref(fast_ms), ctypes.byref(exact_ms)))
        return bool(last.value), steps.value, would.value, fast_ms.value, exact_ms.value

    def set_estep_dictionary(self, mode):
        """'never' | 'auto' (default: tried for genotype tables computed without a beta addition) | 'always' (tried for
        every E-step).  Bit-identical results in every mode; include/demux_hip.h: dmx_set_estep_dictionary."""
        check(self._lib.dmx_set_estep_dictionary(self._h, {'never': 0, 'auto': 1, 'always': 2}[mode]))

    def estep_form(self):
        """(form, distinct) of the last E-step: form 'direct' | 'packed' | 'dict' | 'dict_block' | None, distinct = most distinct
        values in a row of genotype_prob as counted by the last dictionary build (0: none was tried, 9: too many)."""
        form, distinct = ctypes.c_int32(0), ctypes.c_int32(0)
        check(self._lib.dmx_get_estep_form(self._h, ctypes.byref(form), ctypes.byref(distinct)))
        return {0: None, 1: 'direct', 2: 'dict', 3: 'dict_block', 4: 'packed'}[form.value], distinct.value

    def set_estep_packing(self, mode):
        """'never' | 'auto' (default: where it pays) | 'always' (every barcode on packed lane groups) | 'split' (the
        longest barcodes on 64 lanes, the rest packed, whatever their number): several option slots per lane for narrow
        doublet tables (include/demux_hip.h: dmx_set_estep_packing)."""
        check(self._lib.dmx_set_estep_packing(self._h, {'never': 0, 'auto': 1, 'always': 2, 'split': 3}[mode]))

    def set_estep_schedule(self, schedule):
        """'auto' (default: tile-major schedule where it pays), 'tiled' (whenever built), 'direct' (never);
        include/demux_hip.h: dmx_set_estep_schedule."""
        check(self._lib.dmx_set_estep_schedule(self._h, {'direct': 0, 'auto': 1, 'tiled': 2}[schedule]))

    def set_mstep_wide_addresses(self, wide):
        """include/demux_hip.h: dmx_set_mstep_wide_addresses (the M-step form of the largest problems, at any size)."""
        check(self._lib.dmx_set_mstep_wide_addresses(self._h, int(bool(wide))))

    def set_mstep_tiles(self, mode):
        """Tile-major form of the M-step: 'never' | 'auto' (default: when building its records pays, i.e. from 8 M-steps on) |
        'always' (at the first M-step); needs the exact additions off and G <= 64.  include/demux_hip.h: dmx_set_mstep_tiles."""
        if isinstance(mode, str):
            mode = {'never': 0, 'auto': 1, 'always': 2}[mode]
        check(self._lib.dmx_set_mstep_tiles(self._h, int(mode) if not isinstance(mode, bool) else (2 if mode else 0)))

    def set_msteps_expected(self, n):
        """Hint: about n more M-steps will run on the resident problem (include/demux_hip.h: dmx_set_msteps_expected)."""
        check(self._lib.dmx_set_msteps_expected(self._h, int(n)))

    def mstep_tiles_info(self):
        """(the tile-major M-step records exist, host wall time of their build in ms)."""
        built, ms = ctypes.c_int32(0), ctypes.c_double(0)
        check(self._lib.dmx_get_mstep_tiles_info(self._h, ctypes.byref(built), ctypes.byref(ms)))
        return bool(built.value), ms.value

    def mstep_form(self):
        """None | 'items' | 'tiles' | 'items_fixed' (the work items adding the tile-major form's integers, under the incremental
        M-step: calls too short to pay for the tile-major records): the form of the last M-step launch (dmx_get_mstep_form)."""
        form = ctypes.c_int32(0)
        check(self._lib.dmx_get_mstep_form(self._h, ctypes.byref(form)))
        return {0: None, 1: 'items', 2: 'tiles', 3: 'items_fixed'}[form.value]

    def set_live_floor_on_grid(self, on_grid):
        """True (default): an E-step ahead of a fixed-point M-step counts a posterior as live from 2^-26 on - below it the M-step adds
        the integer 0; False: from 2^-80 on, as the float64 forms need it.  Same additions bit for bit
        (include/demux_hip_debug.h: dmx_set_live_floor_on_grid)."""
        check(self._lib.dmx_set_live_floor_on_grid(self._h, int(bool(on_grid))))

    def live_floor(self):
        """(floor of the barcode codes the last E-step - or a rebuild - left, rebuild launches of M-steps since reset_timings)."""
        floor, rebuilds = ctypes.c_float(0), ctypes.c_int64(0)
        check(self._lib.dmx_get_live_floor(self._h, ctypes.byref(floor), ctypes.byref(rebuilds)))
        return floor.value, rebuilds.value

    def debug_live_counts(self):
        """[B] int32: live posteriors of every barcode as its code counts them (G <= 64; dmx_debug_get_live_counts)."""
        out = np.empty(self.B, dtype=np.int32)
        check(self._lib.dmx_debug_get_live_counts(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def redo_count(self):
        """Sums the last exact-mode M-step redid in the reference's order (include/demux_hip.h: dmx_get_redo_count)."""
        n = ctypes.c_int64(0)
        check(self._lib.dmx_get_redo_count(self._h, ctypes.byref(n)))
        return n.value

    def set_exact_additions(self, exact):
        """M-step summation mode (include/demux_hip.h: dmx_set_exact_additions). Default: exact."""
        check(self._lib.dmx_set_exact_additions(self._h, int(bool(exact))))

    # ---- instrumentation ----------------------------------------------------------------
    def set_phase_timers(self, on):
        """HIP events around the phases of the calls that follow, read by timings() (default off - an event record is a barrier
        packet of its own, 6 us per phase boundary; the launch counts are kept either way: include/demux_hip.h dmx_set_phase_timers)."""
        check(self._lib.dmx_set_phase_timers(self._h, int(bool(on))))

    def timings(self):
        """{phase: {ms, launches}} since reset_timings(); ms only of the phases that ran with set_phase_timers(True), -1 when
        the phase ran but never with the timers on (dmx_get_timings)."""
        ms = (ctypes.c_double * _lib.T_COUNT)()
        n = (ctypes.c_int64 * _lib.T_COUNT)()
        check(self._lib.dmx_get_timings(self._h, ms, n))
        return {name: dict(ms=ms[i], launches=int(n[i])) for i, name in enumerate(_lib.TIMER_NAMES)}

    def reset_timings(self):
        check(self._lib.dmx_reset_timings(self._h))

    def trim_cache(self):
        """Give the device blocks this context keeps for re-use back to the driver; returns the bytes released
        (include/demux_hip.h: dmx_trim_cache)."""
        n = ctypes.c_int64(0)
        check(self._lib.dmx_trim_cache(self._h, ctypes.byref(n)))
        return n.value

    def release_problem(self):
        """The resident problem (and any staged containers) back into this context's block cache
        (include/demux_hip.h: dmx_release_problem)."""
        self._resident_key = None  # (demux.py: _pack_on_device keeps the packed problem of the shared context across calls)
        check(self._lib.dmx_release_problem(self._h))
        self.B = self.V = self.G = self.N = self.K = 0

    def device_bytes(self):
        n = ctypes.c_int64(0)
        check(self._lib.dmx_device_bytes(self._h, ctypes.byref(n)))
        return n.value

    # ---- device self-tests (numpy-exact float32 building blocks) -------------------------
    def test_log(self, x):
        x = as_c(x, np.float32)
        out = np.empty_like(x)
        check(self._lib.dmx_test_logf(self._h, ptr(x), ptr(out), x.size))
        return out

    def test_log_hot(self, x):
        x = as_c(x, np.float32)
        out = np.empty_like(x)
        check(self._lib.dmx_test_logf_hot(self._h, ptr(x), ptr(out), x.size))
        return out

    def test_log2_hw(self, x):
        x = as_c(x, np.float32)
        out = np.empty_like(x)
        check(self._lib.dmx_test_log2_hw(self._h, ptr(x), ptr(out), x.size))
        return out

    def test_exp(self, x):
        x = as_c(x, np.float32)
        out = np.empty_like(x)
        check(self._lib.dmx_test_expf(self._h, ptr(x), ptr(out), x.size))
        return out

    def test_softmax(self, x):
        x = as_c(x, np.float32)
        out = np.empty_like(x)
        check(self._lib.dmx_test_softmax(self._h, ptr(x), ptr(out), x.shape[0], x.shape[1]))
        return out


_contexts = {}
_contexts_lock = threading.RLock()


def default_device():
    """GPU used by the Demultiplexer front-end: DEMUXALOT_AMD_DEVICE (taken as is), else LOCAL_RANK, else 0.
    Launchers often set HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES per rank as well, so that every rank sees
    ONE GPU as ordinal 0 while LOCAL_RANK still counts up: LOCAL_RANK is therefore folded into the visible
    device count."""
    if os.environ.get('DEMUXALOT_AMD_DEVICE', '') != '':
        return int(os.environ['DEMUXALOT_AMD_DEVICE'])
    if os.environ.get('LOCAL_RANK', '') != '':
        n = _lib.device_count()
        return int(os.environ['LOCAL_RANK']) % n if n > 0 else 0
    return 0


def get_context(device=None) -> DeviceContext:
    """Process-wide cached context per device. Raises when no GPU is visible (no CPU fallback).
    The cached context holds ONE resident problem: callers that keep state on the GPU across calls of other
    entry points (the staged_genotype_learning generator, DevicePosteriors) own a private DeviceContext
    instead, and the Demultiplexer entry points that use this one serialise on `shared_context_lock`."""
    device = default_device() if device is None else int(device)
    with _contexts_lock:
        if device not in _contexts:
            _contexts[device] = DeviceContext(device)
            _contexts[device]._is_shared = True  # (demux.py: _pack_on_device keeps its packed problem across calls)
        return _contexts[device]


shared_context_lock = threading.RLock()


def shared_contexts():
    """The process-wide contexts created so far, one per device (demux.py: invalidate_resident)."""
    with _contexts_lock:
        return list(_contexts.values())

# Private contexts (a DevicePosteriors, a staged_genotype_learning generator) come from a small pool: a context that
# has been used keeps its stream and, through the runtime's allocator, the address ranges of its buffers, and
# installing the next problem on it costs what it costs on the shared context; a brand-new context pays for fresh
# multi-gigabyte allocations first (predict_posteriors(on_device=True) at 200k x 100k x 64: 0.73 s against 0.31 s).
_idle_private = {}
_PRIVATE_POOL = 2


def acquire_private_context(device=None) -> DeviceContext:
    device = default_device() if device is None else int(device)
    with _contexts_lock:
        idle = _idle_private.get(device)
        ctx = idle.pop() if idle else None
    if ctx is None:
        return DeviceContext(device)
    ctx.apply_environment()
    ctx.set_keep_molecule_calls(False)
    return ctx


def release_private_context(ctx, failed=False):
    """Back to the pool, its resident problem released into its block cache (the next problem installed on it re-uses the
    blocks; an allocation that runs out of device memory anywhere in the process gives the parked blocks of every context
    back first: csrc/dmx_api.cpp ctx_malloc).  `failed`: the holder is unwinding from an exception - the context, which
    may carry a sticky HIP error, is destroyed instead.  The pool holds two contexts per device; drain_private_contexts()
    empties it, trim_device_caches() returns every parked block of a device to the driver."""
    if ctx is None or getattr(ctx, '_h', None) is None:
        return
    if not failed:
        try:
            ctx.release_problem()
        except Exception:  # noqa: BLE001 - a context that cannot even release is not worth keeping
            failed = True
    if not failed:
        with _contexts_lock:
            idle = _idle_private.setdefault(ctx.device, [])
            if len(idle) < _PRIVATE_POOL:
                idle.append(ctx)
                return
    ctx.close()


def drain_private_contexts():
    """Destroys the pooled private contexts (their blocks go to the device's retired list; trim_device_caches() frees those)."""
    with _contexts_lock:
        pooled = [ctx for idle in _idle_private.values() for ctx in idle]
        _idle_private.clear()
    for ctx in pooled:
        ctx.close()


def trim_device_caches(device=None):
    """Every device block this process keeps parked on `device` - idle blocks of all live contexts, blocks of destroyed
    ones - back to the driver; returns the bytes (include/demux_hip.h: dmx_trim_device_caches)."""
    device = default_device() if device is None else int(device)
    n = ctypes.c_int64(0)
    check(_lib.load().dmx_trim_device_caches(device, ctypes.byref(n)))
    return n.value
