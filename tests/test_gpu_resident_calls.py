"""Resident call sets on the GPU (include/demux_hip_debug.h "Resident calls"; DESIGN.md "Resident calls"): the records a count
leaves in a set against the reference's recorded records, upload / concatenate / counts at the kernels' block tails, the
Demultiplexer and the detection on ResidentCalls against the reference's recorded outputs, and the sets' life cycle.  What the
tests rest on is the byte counter of the call records (DeviceContext.calls_transfer_bytes): the resident path must not move it."""
import numpy as np
import pytest

from demuxalot_amd import (BarcodeHandler, CompressedSNPCalls, DecodedReads, Demultiplexer, ProbabilisticGenotypes, ReadCounter,
                           ResidentCalls, ResidentReads, calls_per_barcode, count_snps_from_read_chunks, count_snps_from_reads,
                           detect_snps_positions_from_calls, detect_snps_positions_from_reads, summarize_counted_SNPs)
from demuxalot_amd._lib import DemuxHipError
from demuxalot_amd.device import DeviceContext, get_context, shared_context_lock
from demuxalot_amd.snp_counter import MOLECULE_DTYPE, SNP_CALL_DTYPE, _container, quality_table
from tests import fixture_io as fio
from tests.test_count_reads_cpu import FIXTURES, assert_records_equal, fixture_chromosomes, small_problem
from tests.test_count_reads_stream_cpu import chunkings
from tests.test_coverage_cpu import FIXTURE as F10, fixture_reads, threshold_kwargs

pytestmark = pytest.mark.gpu

INVALID = r'status -1\)'  # DMX_ERR_INVALID


def record_bytes(calls):
    return 12 * calls.n_molecules + 13 * calls.n_snp_calls


def random_container(n_calls, n_molecules, n_barcodes=50, seed=0):
    rng = np.random.default_rng(seed + 1000 * n_calls + n_molecules)
    return CompressedSNPCalls.from_arrays(
        rng.integers(0, n_barcodes, n_molecules), rng.integers(0, max(1, n_molecules), n_calls), rng.integers(0, 10 ** 6, n_calls),
        rng.integers(0, 4, n_calls), rng.random(n_calls).astype(np.float32), compressed_ub=rng.integers(0, 2 ** 31 - 1, n_molecules),
        p_group_misaligned=rng.random(n_molecules).astype(np.float32))


def assert_same_container(got, want, what):
    assert (got.n_molecules, got.n_snp_calls) == (want.n_molecules, want.n_snp_calls), what
    assert_records_equal(got.molecules, want.molecules[:want.n_molecules], f'{what}: molecules')
    assert_records_equal(got.snp_calls, want.snp_calls[:want.n_snp_calls], f'{what}: snp_calls')


# ---- 1. records --------------------------------------------------------------------------------------------------------------
STEPS = ('one-shot', 'max_reads_per_call=1', 'max_reads_per_call=7', 'max_reads_per_call=64')
# (count_snps_from_read_chunks takes host chunks; the device ranges of a ResidentReads are the max_reads_per_call forms)
FORMS = [(form, 'host') for form in STEPS] + [(form, 'device') for form in STEPS] + [('chunks', 'host')]


@pytest.mark.parametrize('form,reads_on', FORMS)
@pytest.mark.parametrize('name', FIXTURES)
def test_counted_records_stay_on_the_device_and_equal_the_reference(name, form, reads_on):
    chromosomes = fixture_chromosomes(name)
    decoded = {chromosome: DecodedReads(**reads) for chromosome, reads, *_ in chromosomes}
    positions = {chromosome: p for chromosome, _reads, p, *_ in chromosomes}
    positions['no reads here'] = next(iter(positions.values()))[:3]
    want = {chromosome: (molecules, snp_calls) for chromosome, _r, _p, molecules, snp_calls in chromosomes}
    ctx = get_context()
    resident_reads = {chromosome: ResidentReads(reads) for chromosome, reads in decoded.items()} if reads_on == 'device' else None
    try:
        before = ctx.calls_transfer_bytes()
        if form == 'chunks':
            def chunks_of(reads):  # a generator: consumed lazily, with empty chunks at the front, in the middle and at the end
                cuts = [0] + chunkings(reads.n_reads)['empty chunks'] + [reads.n_reads]
                return (reads.slice(lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:]))
            counted = count_snps_from_read_chunks({c: chunks_of(reads) for c, reads in decoded.items()}, positions, resident_calls=True)
        else:
            step = None if form == 'one-shot' else int(form.split('=')[1])
            counted = count_snps_from_reads(resident_reads or decoded, positions, max_reads_per_call=step, resident_calls=True)
        assert ctx.calls_transfer_bytes() == before, 'counting into resident sets moved call records over the link'
        assert list(counted) == list(positions) and all(isinstance(calls, ResidentCalls) for calls in counted.values())
        empty = counted.pop('no reads here')
        assert (empty.n_molecules, empty.n_snp_calls, empty.closed) == (0, 0, False) and empty.to_host().n_snp_calls == 0
        assert ctx.calls_transfer_bytes() == before
        frame = summarize_counted_SNPs(counted)
        for chromosome, calls in counted.items():
            molecules, snp_calls = want[chromosome]
            assert tuple(frame.loc[chromosome]) == (calls.n_molecules, calls.n_snp_calls) == (len(molecules), len(snp_calls))
            assert calls.nbytes >= record_bytes(calls)
            at = ctx.calls_transfer_bytes()
            host = calls.to_host()
            moved = ctx.calls_transfer_bytes()
            assert (moved[0] - at[0], moved[1] - at[1]) == (0, 12 * len(molecules) + 13 * len(snp_calls)), 'to_host() is the one download'
            assert_records_equal(host.molecules, molecules, f'{name} {chromosome} {form} molecules')
            assert_records_equal(host.snp_calls, snp_calls, f'{name} {chromosome} {form} snp_calls')
        for calls in list(counted.values()) + [empty]:
            calls.close()
    finally:
        for resident in (resident_reads or {}).values():
            resident.close()


@pytest.mark.parametrize('name', FIXTURES)
def test_a_read_counter_that_keeps_its_calls_appends_nothing_for_a_push_that_emits_nothing(name):
    for chromosome, reads, positions, molecules, snp_calls in fixture_chromosomes(name):
        reads = DecodedReads(**reads)
        bounds = [0] + chunkings(reads.n_reads)['39 single reads'] + [reads.n_reads]
        emitted = []
        with ReadCounter(positions, keep_calls=True) as counter:
            before = counter._ctx.calls_transfer_bytes()
            for lo, hi in zip(bounds[:-1], bounds[1:]):
                emitted.append(counter.push(reads.slice(lo, hi)))
                assert counter.calls is None
            emitted.append(counter.push(None))  # an empty push in the middle of the stream
            emitted.append(counter.finish())
            assert counter._ctx.calls_transfer_bytes() == before
        calls = counter.calls
        assert (0, 0) in emitted[:-1], 'the chunking must include pushes that emit nothing'
        assert all(isinstance(m, int) and isinstance(c, int) for m, c in emitted)
        assert (sum(m for m, _ in emitted), sum(c for _, c in emitted)) == (calls.n_molecules, calls.n_snp_calls)
        assert_same_container(calls.to_host(), _container(molecules, snp_calls), f'{name} {chromosome}')
        calls.close()
    # a counter left before finish() leaves no set behind, and the default still returns arrays
    with ReadCounter(positions, keep_calls=True) as counter:
        counter.push(reads.slice(0, 5))
    assert counter.calls is None
    with ReadCounter(positions) as counter:
        part = counter.finish(reads)
    assert part[0].dtype == MOLECULE_DTYPE and part[1].dtype == SNP_CALL_DTYPE and counter.calls is None


# ---- 2. upload, round trip, edges --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_calls,n_molecules', [(0, 0), (0, 1), (1, 1), (255, 1), (256, 3), (257, 40), (0, 257), (513, 256)])
def test_upload_round_trip_at_the_block_tails(n_calls, n_molecules):
    container = random_container(n_calls, n_molecules)
    ctx = get_context()
    before = ctx.calls_transfer_bytes()
    with ResidentCalls(container) as resident:
        assert ctx.calls_transfer_bytes() == (before[0] + record_bytes(container), before[1])
        assert (resident.n_molecules, resident.n_snp_calls) == (n_molecules, n_calls) and not resident.closed
        assert_same_container(resident.to_host(), container, f'{n_calls} calls, {n_molecules} molecules')
        assert ctx.calls_transfer_bytes() == (before[0] + record_bytes(container), before[1] + record_bytes(container))
    assert resident.closed
    with pytest.raises(RuntimeError, match='closed'):
        resident.to_host()
    # a container with a spare tail: only the first n records are the set
    padded = CompressedSNPCalls(start_snps_size=n_calls + 5, start_molecule_size=n_molecules + 2)
    padded.snp_calls[:n_calls], padded.molecules[:n_molecules] = container.snp_calls, container.molecules
    padded.n_snp_calls, padded.n_molecules = n_calls, n_molecules
    with ResidentCalls(padded) as resident:
        assert_same_container(resident.to_host(), container, 'padded')


@pytest.mark.parametrize('n_calls', [1, 256, 257])
@pytest.mark.parametrize('bad_index', [-1, 'n_molecules'])
def test_upload_refuses_a_molecule_index_outside_the_table_as_staging_does(n_calls, bad_index):
    container = random_container(n_calls, 9)
    container.snp_calls['molecule_index'][n_calls - 1] = -1 if bad_index == -1 else container.n_molecules
    with shared_context_lock:
        ctx = get_context()
        with pytest.raises(DemuxHipError, match=INVALID) as staged:
            ctx.stage_containers([(0, container.snp_calls, container.molecules)])
    with pytest.raises(DemuxHipError, match=INVALID) as uploaded:
        ResidentCalls(container)
    assert str(uploaded.value) == str(staged.value) and 'molecule_index outside the molecule table' in str(uploaded.value)
    # calls without a molecule table: refused before anything is copied, as staging refuses them
    orphan = random_container(3, 1)
    orphan.molecules, orphan.n_molecules = orphan.molecules[:0], 0
    with shared_context_lock:
        with pytest.raises(DemuxHipError, match=INVALID) as staged:
            ctx.stage_containers([(0, orphan.snp_calls, orphan.molecules)])
    with pytest.raises(DemuxHipError, match=INVALID) as uploaded:
        ResidentCalls(orphan)
    assert str(uploaded.value) == str(staged.value)
    # the context is as usable as before
    good = random_container(n_calls, 9)
    with ResidentCalls(good) as resident:
        assert_same_container(resident.to_host(), good, 'after the refusals')


# ---- 3. concatenate ----------------------------------------------------------------------------------------------------------
def test_concatenate_is_the_host_concatenate_on_the_device(monkeypatch):
    parts = [random_container(257, 40, seed=1), random_container(0, 0), random_container(300, 7, seed=2)]
    want = CompressedSNPCalls.concatenate(parts)
    ctx = get_context()
    resident = [ResidentCalls(part) for part in parts]
    before = ctx.calls_transfer_bytes()
    joined = ResidentCalls.concatenate(resident)
    assert ctx.calls_transfer_bytes() == before
    assert joined._handle not in [part._handle for part in resident] and joined._ctx is ctx
    assert (joined.n_molecules, joined.n_snp_calls) == (47, 557)
    assert_same_container(joined.to_host(), want, 'three parts, the middle one empty')
    for part, host in zip(resident, parts):  # the parts are untouched
        assert_same_container(part.to_host(), host, 'a part after the concatenate')
    # other shapes: one part, an empty part with molecules in front, the same set twice
    for shape in ([0], [1], [1, 0], [2, 2], [1, 2, 0, 1]):
        again = ResidentCalls.concatenate([resident[k] for k in shape])
        assert_same_container(again.to_host(), CompressedSNPCalls.concatenate([parts[k] for k in shape]), str(shape))
        again.close()
    only_molecules = ResidentCalls(random_container(0, 5))
    mixed = ResidentCalls.concatenate([only_molecules, resident[0]])
    assert_same_container(mixed.to_host(), CompressedSNPCalls.concatenate([random_container(0, 5), parts[0]]), 'molecules without calls in front')
    # 2^31 molecules cannot be built (24 GB of records): the bound is tested on the host side of the entry point, with the
    # sizes the sets report
    monkeypatch.setitem(resident[0]._info, 'n_molecules', 2 ** 31 - 7)
    with pytest.raises(ValueError, match='2\\^31 molecules'):
        ResidentCalls.concatenate([resident[0], resident[2]])
    monkeypatch.setitem(resident[0]._info, 'n_molecules', 2 ** 31 - 8)
    ResidentCalls.concatenate([resident[0], resident[2]]).close()  # (2^31 - 1 in the books is not refused; the device holds 47)
    monkeypatch.undo()
    # a closed part, a part of another context
    other_ctx = DeviceContext(0)
    try:
        foreign = ResidentCalls(parts[0], on_context=other_ctx)
        with pytest.raises(ValueError, match='one context'):
            ResidentCalls.concatenate([resident[0], foreign])
        with pytest.raises(DemuxHipError, match=INVALID):
            ctx.calls_concatenate([resident[0]._handle, foreign._handle])
        foreign.close()
    finally:
        other_ctx.close()
    resident[2].close()
    with pytest.raises(RuntimeError, match='closed'):
        ResidentCalls.concatenate(resident)
    for calls in resident + [joined, only_molecules, mixed]:
        calls.close()


# ---- 4. counts ---------------------------------------------------------------------------------------------------------------
def numpy_counts(container, n_barcodes):
    cb = container.molecules['compressed_cb'][:container.n_molecules]
    return (np.bincount(cb[container.snp_calls['molecule_index'][:container.n_snp_calls]], minlength=n_barcodes),
            np.bincount(cb, minlength=n_barcodes))


def test_barcode_counts_equal_numpy():
    fx = fio.load('f6_shipped_example.npz')
    host, _genotypes, handler = fio.product_inputs(fx)
    B = handler.n_barcodes
    ctx = get_context()
    resident = {chromosome: ResidentCalls(calls) for chromosome, calls in host.items()}
    before = ctx.calls_transfer_bytes()
    for chromosome, calls in resident.items():
        got = calls.barcode_counts(B)
        assert got[0].dtype == np.int64 and got[1].dtype == np.int64
        assert np.array_equal(got[0], numpy_counts(host[chromosome], B)[0]) and np.array_equal(got[1], numpy_counts(host[chromosome], B)[1])
    on_device, on_host = calls_per_barcode(resident, B), calls_per_barcode(host, B)
    assert np.array_equal(on_device[0], on_host[0]) and np.array_equal(on_device[1], on_host[1]) and on_host[0].sum() > 0
    assert summarize_counted_SNPs(resident).equals(summarize_counted_SNPs(host))
    assert ctx.calls_transfer_bytes() == before, 'the counts downloaded records'
    for calls in resident.values():
        calls.close()
    # one barcode holds every call but one (contended atomics), barcode B - 1 holds that one; several blocks
    B, n_molecules, n_calls = 300, 1000, 100_001
    cb = np.full(n_molecules, 5)
    cb[-1] = B - 1
    molecule_index = np.random.default_rng(4).integers(0, n_molecules - 1, n_calls)
    molecule_index[n_calls // 2] = n_molecules - 1
    heavy = CompressedSNPCalls.from_arrays(cb, molecule_index, np.arange(n_calls), np.zeros(n_calls), np.full(n_calls, 0.01))
    with ResidentCalls(heavy) as resident:
        calls, transcripts = resident.barcode_counts(B)
        assert np.array_equal(calls, numpy_counts(heavy, B)[0]) and np.array_equal(transcripts, numpy_counts(heavy, B)[1])
        assert (calls[5], calls[B - 1], calls.sum()) == (n_calls - 1, 1, n_calls) and (transcripts[5], transcripts[B - 1]) == (n_molecules - 1, 1)
        more = resident.barcode_counts(B + 10)
        assert np.array_equal(more[0][:B], calls) and not more[0][B:].any() and not more[1][B:].any()
        with pytest.raises(DemuxHipError, match=INVALID) as refused:  # compressed_cb == n_barcodes
            resident.barcode_counts(B - 1)
        assert 'compressed_cb outside [0, n_barcodes)' in str(refused.value)
        with pytest.raises(DemuxHipError, match=INVALID):
            resident.barcode_counts(0)
        assert np.array_equal(resident.barcode_counts(B)[0], calls)  # (the context is as usable as before)
    with ResidentCalls(random_container(0, 0)) as empty:
        assert not empty.barcode_counts(4)[0].any() and empty.barcode_counts(0)[0].shape == (0,)


# ---- 5. the Demultiplexer, against the reference's recorded outputs -----------------------------------------------------------------
def count_packs(monkeypatch):
    packs = []
    original = DeviceContext.pack_staged_and_set_problem
    monkeypatch.setattr(DeviceContext, 'pack_staged_and_set_problem', lambda self, *a, **k: (packs.append(1), original(self, *a, **k))[1])
    return packs


def check_bitwise(logits, probs, fx, prefix, what):
    fio.assert_bitwise(np.asarray(logits), fx[f'{prefix}_logits'], f'{what} logits')
    fio.assert_bitwise(np.asarray(probs), fx[f'{prefix}_probs'], f'{what} posteriors')


@pytest.mark.parametrize('name', ['f1_synthetic_default.npz', 'f2_synthetic_g4.npz', 'f6_shipped_example.npz'])
def test_predict_and_learn_on_resident_calls_equal_the_reference_and_upload_nothing(name):
    """The expectations tests/test_gpu_parity.py and tests/test_gpu_caches.py hold the host path to, in the mode the suite pins
    (bit-exact).  f4_doublet_penalties.npz records no containers: it pins the penalties of the doublet runs below."""
    fx, f4 = fio.load(name), fio.load('f4_doublet_penalties.npz')
    host, genotypes, handler = fio.product_inputs(fx)
    ctx = get_context()
    resident = {chromosome: ResidentCalls(calls) for chromosome, calls in host.items()}
    before = ctx.calls_transfer_bytes()
    for i in range(int(fx['n_predict'])):
        dp, clip = float(fx[f'predict{i}_dp']), float(fx[f'predict{i}_clip'])
        logits_df, probs_df = Demultiplexer.predict_posteriors(resident, genotypes, handler, p_genotype_clip=clip, doublet_prior=dp)
        assert logits_df.index.name == 'BARCODE' and list(probs_df.columns) == [str(c) for c in fx[f'predict{i}_columns']]
        check_bitwise(logits_df.values, probs_df.values, fx, f'predict{i}', f'{name} predict {i}')
        recorded = f'G{genotypes.n_genotypes}_dp{dp}'
        if recorded in f4:
            fio.assert_bitwise(Demultiplexer._doublet_penalties(genotypes.n_genotypes, dp), f4[recorded], recorded)
    for i in range(int(fx['n_em'])):
        kwargs = dict(n_iterations=int(fx[f'em{i}_n_iterations']), p_genotype_clip=float(fx[f'em{i}_clip']), doublet_prior=float(fx[f'em{i}_dp']))
        prior = fx.get(f'em{i}_prior_logits')
        learnt, last = Demultiplexer.learn_genotypes(resident, genotypes, handler, barcode_prior_logits=None if prior is None else prior.copy(), **kwargs)
        fio.assert_bitwise(learnt.variant_betas, fx[f'em{i}_learnt_betas'], f'{name} run {i} learnt betas')
        fio.assert_bitwise(last.values, fx[f'em{i}_it{kwargs["n_iterations"] - 1}_probs'], f'{name} run {i} last posteriors')
        stages = list(Demultiplexer.staged_genotype_learning(resident, genotypes, handler,
                                                             barcode_prior_logits=None if prior is None else prior.copy(), **kwargs))
        for it, (probs_df, dbg) in enumerate(stages):
            check_bitwise(dbg['barcode_logits'], probs_df.values, fx, f'em{i}_it{it}', f'{name} run {i} it {it}')
            fio.assert_bitwise(dbg['genotype_addition'], fx[f'em{i}_it{it}_addition'], 'addition')
            fio.assert_bitwise(dbg['genotype_prior'], fx['pack1_betas'], 'prior')
    assert ctx.calls_transfer_bytes() == before, 'the resident path moved call records'
    # the public host twin takes to_host() of the sets
    v2snp, betas, molecule_calls, barcode_calls = Demultiplexer.pack_calls(resident, genotypes, add_data_prior=True)
    fio.assert_bitwise(betas, fx['pack1_betas'], 'pack_calls betas')
    assert np.array_equal(barcode_calls['variant_id'], fx['pack_bc_variant_id']) and len(molecule_calls) == int(fx['pack_n_molecule_calls'])
    assert ctx.calls_transfer_bytes() == (before[0], before[1] + sum(record_bytes(calls) for calls in host.values()))
    for calls in resident.values():
        calls.close()


def test_resident_sets_pack_once_and_are_keyed_by_their_handles(monkeypatch):
    fx = fio.load('f1_synthetic_default.npz')
    host, genotypes, handler = fio.product_inputs(fx)
    packs = count_packs(monkeypatch)
    ctx = get_context()
    ctx._resident_key = None
    dp, clip = float(fx['predict0_dp']), float(fx['predict0_clip'])
    resident = {chromosome: ResidentCalls(calls) for chromosome, calls in host.items()}
    before = ctx.calls_transfer_bytes()

    def predict(calls):
        logits_df, probs_df = Demultiplexer.predict_posteriors(calls, genotypes, handler, p_genotype_clip=clip, doublet_prior=dp)
        check_bitwise(logits_df.values, probs_df.values, fx, 'predict0', 'predict')

    def learn(calls):
        kwargs = dict(n_iterations=int(fx['em0_n_iterations']), p_genotype_clip=float(fx['em0_clip']), doublet_prior=float(fx['em0_dp']))
        learnt, last = Demultiplexer.learn_genotypes(calls, genotypes, handler, **kwargs)
        fio.assert_bitwise(last.values, fx[f'em0_it{kwargs["n_iterations"] - 1}_probs'], 'learn posteriors')
        fio.assert_bitwise(learnt.variant_betas, fx['em0_learnt_betas'], 'learnt betas')

    predict(resident)
    assert len(packs) == 1 and ctx._resident_key[0] == 'resident-calls'
    assert ctx._resident_key[1] == tuple((chromosome, calls._handle) for chromosome, calls in resident.items())
    learn(resident)
    predict(resident)
    assert len(packs) == 1, 'the same sealed sets were packed again'
    # a concatenated or re-uploaded copy has a new handle: it packs again (nothing is hashed to find out that it need not)
    name = next(iter(resident))
    copies = dict(resident)
    copies[name] = ResidentCalls.concatenate([resident[name]])
    predict(copies)
    assert len(packs) == 2
    predict(copies)
    assert len(packs) == 2
    copies[name].close()
    copies[name] = ResidentCalls(host[name])
    uploaded = record_bytes(host[name])
    predict(copies)
    assert len(packs) == 3
    predict(resident)
    assert len(packs) == 4
    assert ctx.calls_transfer_bytes() == (before[0] + uploaded, before[1])
    # host containers of the same records: another key, the host path, the same bits
    predict(host)
    assert len(packs) == 5 and ctx._resident_key[0] == 'full'
    predict(resident)
    assert len(packs) == 6
    # the switch
    monkeypatch.setenv('DEMUXALOT_AMD_RESIDENT', '0')
    predict(resident)
    predict(resident)
    assert len(packs) == 8 and ctx._resident_key is None
    monkeypatch.delenv('DEMUXALOT_AMD_RESIDENT')
    predict(resident)
    assert len(packs) == 9
    # a mixed dict
    mixed = dict(resident)
    mixed[name] = host[name]
    for call in (lambda: predict(mixed), lambda: learn(mixed), lambda: Demultiplexer.predict_posteriors(mixed, genotypes, handler, on_device=True),
                 lambda: next(Demultiplexer.staged_genotype_learning(mixed, genotypes, handler))):
        with pytest.raises(TypeError, match='mixes ResidentCalls and host containers'):
            call()
    # a closed set: the next call raises and does not fall back on the resident problem, which IS the one of these handles
    predict(resident)
    assert len(packs) == 9
    kept_key = ctx._resident_key
    assert kept_key[1] == tuple((chromosome, calls._handle) for chromosome, calls in resident.items())
    resident[name].close()
    with pytest.raises(RuntimeError, match='closed'):
        predict(resident)
    with pytest.raises(RuntimeError, match='closed'):
        learn(resident)
    assert len(packs) == 9 and ctx._resident_key == kept_key
    resident[name] = ResidentCalls(host[name])
    predict(resident)
    assert len(packs) == 10
    # calls on a chromosome without variants: the reference's assertion, from n_snp_calls
    stray = dict(resident)
    stray['no variants here'] = ResidentCalls(random_container(3, 2))
    with pytest.raises(AssertionError):
        predict(stray)
    stray['no variants here'].close()
    stray['no variants here'] = ResidentCalls(random_container(0, 2))
    predict(stray)  # (molecules without calls there are fine, as on the host path)
    for calls in list(stray.values()) + [copies[name]]:
        calls.close()


def test_on_device_posteriors_from_sets_of_the_shared_context(monkeypatch):
    """The sets live on the shared context, the posteriors on a pooled one: device pointers are device-wide."""
    from demuxalot_amd import demux
    fx = fio.load('f2_synthetic_g4.npz')
    host, genotypes, handler = fio.product_inputs(fx)
    shared = get_context()
    resident = {chromosome: ResidentCalls(calls) for chromosome, calls in host.items()}
    assert all(calls._ctx is shared for calls in resident.values())
    taken = []
    original = demux.acquire_private_context
    monkeypatch.setattr(demux, 'acquire_private_context', lambda *a, **k: (lambda c: (taken.append((c, c.calls_transfer_bytes())), c)[1])(original(*a, **k)))
    before = shared.calls_transfer_bytes()
    i = 1
    posteriors = Demultiplexer.predict_posteriors(resident, genotypes, handler, p_genotype_clip=float(fx[f'predict{i}_clip']),
                                                  doublet_prior=float(fx[f'predict{i}_dp']), on_device=True)
    with posteriors:
        assert posteriors._ctx is taken[0][0] and posteriors._ctx is not shared
        logits_df, probs_df = posteriors.to_dataframes()
        check_bitwise(logits_df.values, probs_df.values, fx, f'predict{i}', 'on_device predict')
        assert posteriors._ctx.calls_transfer_bytes() == taken[0][1]
    kwargs = dict(n_iterations=int(fx['em0_n_iterations']), p_genotype_clip=float(fx['em0_clip']), doublet_prior=float(fx['em0_dp']))
    learnt, posteriors = Demultiplexer.learn_genotypes(resident, genotypes, handler, on_device=True, **kwargs)
    with posteriors:
        fio.assert_bitwise(learnt.variant_betas, fx['em0_learnt_betas'], 'on_device learnt betas')
        fio.assert_bitwise(posteriors.to_dataframes()[1].values, fx[f'em0_it{kwargs["n_iterations"] - 1}_probs'], 'on_device last posteriors')
    assert shared.calls_transfer_bytes() == before and all(c.calls_transfer_bytes() == at for c, at in taken)
    # the owner may release a set as soon as the call has returned; the posteriors stay
    posteriors = Demultiplexer.predict_posteriors(resident, genotypes, handler, doublet_prior=0.0, on_device=True)
    for calls in resident.values():
        calls.close()
    with posteriors:
        fio.assert_bitwise(posteriors.to_dataframes()[1].values, fx['predict0_probs'], 'posteriors after the sets were released')


# ---- 6. detection ------------------------------------------------------------------------------------------------------------
def f10_inputs(fx):
    """(every read parse_read accepts, the whitelisted ones, genotypes, barcode handler) of the f10 fixture, as
    tests/test_gpu_coverage.py: fixture_inputs builds them."""
    everything, whitelisted = {}, {}
    for i, chrom in enumerate(fx['chroms']):
        reads = fixture_reads(fx, i)
        everything[str(chrom)] = DecodedReads(**reads)
        keep = reads['compressed_cb'] >= 0
        kept = {name: reads[name][keep] for name in ('reference_start', 'compressed_cb', 'compressed_ub', 'p_misaligned',
                                                     'alignment_score', 'cigar_begin', 'n_cigar', 'seq_begin', 'l_seq')}
        whitelisted[str(chrom)] = DecodedReads(cigar=reads['cigar'], seq=reads['seq'], qual=reads['qual'], **kept)
    genotypes = ProbabilisticGenotypes([str(s) for s in fx['genotype_names']], default_prior=float(fx['default_prior']))
    genotypes.var2varid = {(str(c), int(p), 'ACGTN'[int(b)]): int(r)
                           for c, p, b, r in zip(fx['var_chrom'], fx['var_pos'], fx['var_base'], fx['var_row'])}
    genotypes.variant_betas = np.array(fx['betas'], dtype=np.float32)
    return everything, whitelisted, genotypes, BarcodeHandler([str(b) for b in fx['barcodes']])


def f10_kwargs(fx, e):
    s, n_best, n_add, ignore = (int(v) for v in fx['end_to_end'][e])
    kwargs = threshold_kwargs(fx['thresholds'][s])
    del kwargs['minimum_fraction_of_ref_and_alt']  # the reference's detect_snps_positions leaves it at its default
    kwargs.update(n_best_snps_per_donor=n_best, n_additional_best_snps=n_add, ignore_known_snps=bool(ignore))
    return kwargs


def assert_reference_detection(result, fx, e):
    chroms = [str(c) for c in fx['chroms']]
    assert [(c, p) for c, p, *_ in result] == [(chroms[c], int(p)) for c, p in zip(fx[f'detect{e}_chrom'], fx[f'detect{e}_pos'])]
    fio.assert_bitwise(np.stack([imp for _, _, imp, _ in result]), fx[f'detect{e}_importances'], 'importances')
    assert [''.join(bc) for *_, bc in result] == [str(b) for b in fx[f'detect{e}_bases']]
    assert np.array_equal([list(bc.values()) for *_, bc in result], fx[f'detect{e}_totals'])


@pytest.mark.parametrize('e', [0, 1])
def test_detection_from_resident_reads_moves_no_call_record(e, monkeypatch):
    from demuxalot_amd import demux
    fx = fio.load(F10)
    everything, whitelisted, genotypes, handler = f10_inputs(fx)
    chroms = [str(c) for c in fx['chroms']]
    shared = get_context()
    taken = []
    original = demux.acquire_private_context
    monkeypatch.setattr(demux, 'acquire_private_context', lambda *a, **k: (lambda c: (taken.append((c, c.calls_transfer_bytes())), c)[1])(original(*a, **k)))
    resident_everything = {c: ResidentReads(reads, coverage_only=True) for c, reads in everything.items()}
    resident_whitelisted = {c: ResidentReads(reads) for c, reads in whitelisted.items()}
    try:
        before = shared.calls_transfer_bytes()
        sets_before = len(shared_sets(shared))
        result = detect_snps_positions_from_reads(resident_whitelisted, genotypes, handler, coverage_reads=resident_everything,
                                                  chromosome2length={c: int(fx['length']) for c in chroms}, **f10_kwargs(fx, e))
        assert_reference_detection(result, fx, e)
        assert shared.calls_transfer_bytes() == before, 'the shared context moved call records'
        assert len(taken) == 1 and all(c.calls_transfer_bytes() == at for c, at in taken), 'the posteriors\' context moved call records'
        assert len(shared_sets(shared)) == sets_before, 'the detection left its call sets behind'
    finally:
        for resident in list(resident_everything.values()) + list(resident_whitelisted.values()):
            resident.close()
    # host reads: the read passes run on the posteriors' context, the call sets live there, the result is the same
    taken.clear()
    result = detect_snps_positions_from_reads(whitelisted, genotypes, handler, coverage_reads=everything,
                                              chromosome2length={c: int(fx['length']) for c in chroms}, **f10_kwargs(fx, e))
    assert_reference_detection(result, fx, e)
    assert shared.calls_transfer_bytes() == before and all(c.calls_transfer_bytes() == at for c, at in taken)


def shared_sets(ctx):
    """Handles of the call sets a context holds, found by asking for every handle handed out so far."""
    with shared_context_lock:
        probe = ctx.calls_open()
        ctx.calls_release(probe)
        alive = []
        for handle in range(1, probe):
            try:
                ctx.calls_info(handle)
                alive.append(handle)
            except DemuxHipError:
                pass
    return alive


def test_detection_from_resident_calls_equals_the_detection_from_their_host_copies():
    fx = fio.load(F10)
    _everything, whitelisted, genotypes, handler = f10_inputs(fx)
    kwargs = {k: v for k, v in f10_kwargs(fx, 0).items() if k in ('n_best_snps_per_donor', 'n_additional_best_snps', 'ignore_known_snps')}
    shared = get_context()
    known = count_snps_from_reads(whitelisted, genotypes.get_chromosome2positions(), resident_calls=True)
    chroms = [str(c) for c in fx['chroms']]
    candidates = {c: np.unique(np.concatenate([reads.reference_start[::7] + 3, reads.reference_start[::11] + 10,
                                               fx['detect0_pos'][fx['detect0_chrom'] == chroms.index(c)]])).astype(np.int32)
                  for c, reads in whitelisted.items()}
    candidate = count_snps_from_reads(whitelisted, candidates, resident_calls=True)
    assert sum(calls.n_snp_calls for calls in candidate.values()) > 1000
    before = shared.calls_transfer_bytes()
    on_device = detect_snps_positions_from_calls(known, candidate, genotypes, handler, **kwargs)
    assert shared.calls_transfer_bytes() == before
    known_host = {c: calls.to_host() for c, calls in known.items()}
    candidate_host = {c: calls.to_host() for c, calls in candidate.items()}
    on_host = detect_snps_positions_from_calls(known_host, candidate_host, genotypes, handler, **kwargs)
    assert len(on_host) > 0 and [(c, p, bases) for c, p, _i, bases in on_device] == [(c, p, bases) for c, p, _i, bases in on_host]
    fio.assert_bitwise(np.stack([imp for _, _, imp, _ in on_device]), np.stack([imp for _, _, imp, _ in on_host]), 'importances')
    # each of the two may be resident on its own; a dict that mixes the kinds may not
    assert [(c, p) for c, p, *_ in detect_snps_positions_from_calls(known_host, candidate, genotypes, handler, **kwargs)] == [(c, p) for c, p, *_ in on_host]
    mixed = dict(candidate)
    mixed[next(iter(mixed))] = candidate_host[next(iter(mixed))]
    with pytest.raises(TypeError, match='mixes ResidentCalls and host containers'):
        detect_snps_positions_from_calls(known, mixed, genotypes, handler, **kwargs)
    for calls in list(known.values()) + list(candidate.values()):
        calls.close()


# ---- 7. lifetime -------------------------------------------------------------------------------------------------------------
def test_the_sets_are_the_callers_and_handles_are_never_valid_twice():
    container = random_container(300, 20)
    reads, positions = small_problem()
    reads = DecodedReads(**reads) if isinstance(reads, dict) else reads
    with DeviceContext(0) as ctx, DeviceContext(0) as other:
        bytes_before = ctx.device_bytes()
        handle = ctx.calls_upload(container.snp_calls, container.molecules)
        info = ctx.calls_info(handle)
        assert info == dict(n_molecules=20, n_snp_calls=300, nbytes=record_bytes(container), sealed=1)
        assert ctx.device_bytes() == bytes_before, 'dmx_device_bytes counts the problem, not the sets'
        # dmx_release_problem leaves the sets
        ctx.release_problem()
        molecules, snp_calls = ctx.calls_fetch(handle)
        assert_records_equal(molecules, container.molecules, 'molecules after release_problem')
        assert_records_equal(snp_calls, container.snp_calls, 'snp_calls after release_problem')
        # another context's handle, a stale handle, a handle nobody got
        for call in (other.calls_info, other.calls_fetch, other.calls_release, other.calls_seal, other.calls_view, other.calls_append_counted,
                     lambda h: other.calls_barcode_counts(h, 50), lambda h: other.calls_concatenate([h])):
            with pytest.raises(DemuxHipError, match=INVALID):
                call(handle)
        second = other.calls_upload(container.snp_calls, container.molecules)
        assert second > handle
        ctx.calls_release(handle)
        for call in (ctx.calls_info, ctx.calls_fetch, ctx.calls_release, lambda h: ctx.calls_concatenate([h]), lambda h: ctx.calls_info(h + 10 ** 6),
                     lambda h: ctx.calls_info(0), lambda h: ctx.calls_info(-1)):
            with pytest.raises(DemuxHipError, match=INVALID):
                call(handle)
        third = ctx.calls_upload(container.snp_calls, container.molecules)
        assert third > second, 'a handle came back'
        # a sealed set takes no append; an open set cannot be read
        ctx.count_reads(reads, positions, quality_table(), fetch=False)
        with pytest.raises(DemuxHipError, match=INVALID):
            ctx.calls_append_counted(third)
        opened = ctx.calls_open()
        assert ctx.calls_info(opened) == dict(n_molecules=0, n_snp_calls=0, nbytes=0, sealed=0)
        for call in (ctx.calls_fetch, ctx.calls_view, lambda h: ctx.calls_concatenate([h]), lambda h: ctx.calls_barcode_counts(h, 50)):
            with pytest.raises(DemuxHipError, match=INVALID):
                call(opened)
        ctx.calls_append_counted(opened)
        with pytest.raises(DemuxHipError, match=INVALID):  # the same records once more: their molecules do not count on from the set's
            ctx.calls_append_counted(opened)
        ctx.calls_seal(opened)
        want = ctx.count_reads(reads, positions, quality_table())
        got = ctx.calls_fetch(opened)
        assert len(want[0]) > 0 and len(want[1]) > 0
        assert_records_equal(got[0], want[0], 'appended molecules')
        assert_records_equal(got[1], want[1], 'appended snp_calls')
        # nothing counted yet on `other`; and behind a failed push: refused, and the set can still be released
        target = other.calls_open()
        with pytest.raises(DemuxHipError, match=INVALID):
            other.calls_append_counted(target)
        other.count_reads_begin(positions, quality_table())
        assert other.count_reads_push(reads, fetch=False)[0] >= 0
        other.calls_append_counted(target)
        with pytest.raises(DemuxHipError, match=INVALID):  # the chunk starts below the previous chunk's last reference_start
            other.count_reads_push(DecodedReads(**{**reads.arrays(), 'reference_start': reads.reference_start - 1}), fetch=False)
        with pytest.raises(DemuxHipError, match=INVALID):
            other.calls_append_counted(target)
        other.calls_release(target)
        other.count_reads_end()
        with pytest.raises(DemuxHipError, match=INVALID):
            other.calls_info(target)
        # device views are checked: host memory is refused, sizes beyond the allocation are refused
        view = ctx.calls_view(third)
        ctx.stage_device_containers([(0, view)])
        other.stage_device_containers([(0, view)])  # (another context of the same device)
        host_view = type(view)(container.snp_calls.ctypes.data, 300, container.molecules.ctypes.data, 20, 0)
        too_long = type(view)(view.snp_calls, 10 ** 9, view.molecules, 20, 0)
        for bad in (host_view, too_long):
            with pytest.raises(DemuxHipError, match=INVALID):
                ctx.stage_device_containers([(0, bad)])
            with pytest.raises(DemuxHipError, match=INVALID):
                ctx.snp_count_device([(0, bad)], np.zeros(50, np.int32), 1)
        ctx.release_problem()
        other.release_problem()
    # dmx_destroy freed what was left: a ResidentCalls of a destroyed context says so
    with DeviceContext(0) as ctx:
        resident = ResidentCalls(container, on_context=ctx)
        assert resident._ctx is ctx and not resident._shared
    with pytest.raises(RuntimeError, match='destroyed'):
        resident.to_host()
    resident.close()
