"""TEST INFRASTRUCTURE: pack problems at the edges of the device pack's kernels (csrc/repack_device.hip: k_table_insert,
k_match, the compaction, the radix sort, k_heads / k_products, k_variant_counts, k_flatten_container, k_remap_chrom)
and what the reference computes from them.

  make(case)                 one problem: variant keys, the molecule calls as flat arrays in the reference's order
                             (container after container, then call order) and the same calls as CompressedSNPCalls
                             containers; CASES is the table of cases, problem(name) a cached make(CASES[name])
  expected(problem, oracle)  a dict lookup of (chromosome, position, base) + oracle.dedupe_calls + np.bincount, exactly
                             as tests/sanitizer_driver.py: fuzz_pack - nothing here comes from the library
  cases_hit(problem, want)   a Counter of the named cases a problem holds, from its inputs and the oracle's output

The generator restates the hash of the device's variant table (slot_of in repack_device.hip) to CHOOSE variant keys
that land in the table's last slot, so that the linear probe has to wrap; the expected values never use it."""
import collections
import functools
import types

import numpy as np

G = 5                       # genotypes of every problem (the pack does not depend on it)
POS_MAX = 2 ** 31 - 1
TINY = np.float32(1.17549435e-38)  # smallest normal float32
RUN_LENGTHS = (1, 2, 3, 8, 40)

# ---- the cases ------------------------------------------------------------------------------------------------------
# V variants, n_calls molecule calls of which n_matched hit a variant (default: about 70 %), n_barcodes barcodes.
# runs: 'mixed' (runs of 1, 2, 3, 8 and 40 members), 'one' (every call in one run), 'unique' (every call its own run);
# long: one run of 5000 members; float_edges: runs with subnormal / zero products and the members 0, 1 and 1e-38.
CASES = {
    'n0':           dict(seed=1, V=33, n_calls=0, n_barcodes=2),
    'n1_m1':        dict(seed=2, V=1, n_calls=1, n_matched=1, n_barcodes=1),
    'n255_m0':      dict(seed=3, V=2, n_calls=255, n_matched=0, n_barcodes=2),
    'n256_m256':    dict(seed=4, V=31, n_calls=256, n_matched=256, n_barcodes=256),
    'n257_m257':    dict(seed=5, V=32, n_calls=257, n_matched=257, n_barcodes=257),
    'n511':         dict(seed=6, V=33, n_calls=511, n_barcodes=4097),
    'n512':         dict(seed=7, V=1023, n_calls=512, n_barcodes=256),
    'n513_m256':    dict(seed=8, V=1024, n_calls=513, n_matched=256, n_barcodes=257),
    'n700_m1':      dict(seed=9, V=1025, n_calls=700, n_matched=1, n_barcodes=2),
    'edges_v1025':  dict(seed=10, V=1025, n_calls=20000, n_barcodes=4097, float_edges=True),
    'long_v1023':   dict(seed=11, V=1023, n_calls=30000, n_barcodes=257, long=True, float_edges=True),
    'one_run':      dict(seed=12, V=33, n_calls=1500, n_matched=1500, n_barcodes=2, runs='one'),
    'all_unique':   dict(seed=13, V=1025, n_calls=5000, n_matched=5000, n_barcodes=4097, runs='unique'),
    'v32767':       dict(seed=14, V=32767, n_calls=200000, n_barcodes=4097, float_edges=True),
    'v32768':       dict(seed=15, V=32768, n_calls=100000, n_barcodes=256),
    'v65537':       dict(seed=16, V=65537, n_calls=300000, n_barcodes=4097, long=True),
}


# ---- the device table's hash, restated to choose inputs ---------------------------------------------------------------
def table_bits(n_variants):
    """log2 of the slots of the device's variant table: a power of two above 2 V, 64 at least."""
    return max(6, max(1, int(2 * n_variants).bit_length()))


def variant_key(chrom, pos, base):
    chrom, pos, base = (np.asarray(a).astype(np.int64) for a in (chrom, pos, base))
    return ((chrom.astype(np.uint64) & np.uint64(0xFFFFFFFF)) << np.uint64(35)) | (pos.astype(np.uint64) << np.uint64(3)) | base.astype(np.uint64)


def slot_of(key, bits):
    return (key * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(64 - bits)  # uint64 arrays wrap


def _keys_in_last_slot(rng, bits, n_chrom, count):
    found = np.zeros((0, 3), dtype=np.int64)
    while len(found) < count:
        cand = np.stack([rng.integers(0, n_chrom, 1 << 18), rng.integers(1, POS_MAX, 1 << 18), rng.integers(0, 4, 1 << 18)], axis=1)
        hit = slot_of(variant_key(cand[:, 0], cand[:, 1], cand[:, 2]), bits) == np.uint64((1 << bits) - 1)
        found = np.concatenate([found, cand[hit]])
        _, first = np.unique(found[:, 0] << 31 | found[:, 1], return_index=True)  # one key per (chromosome, position)
        found = found[np.sort(first)]
    return found[:count]


# ---- the generator ----------------------------------------------------------------------------------------------------
def _variants(rng, V, n_chrom):
    """V unique (chromosome, position, base) rows in shuffled row order; returns them with the rows of the keys that
    the calls must reach (positions 0 and 2^31 - 1, the keys in the table's last slot) and spare last-slot keys that
    are NO variants."""
    bits = table_bits(V)
    fixed = [(n_chrom - 1, POS_MAX, 3)] + [(0, 0, b) for b in range(5)]   # a multi-allelic site with every base at position 0
    spare = np.zeros((0, 3), dtype=np.int64)
    if V >= 16:
        crafted = _keys_in_last_slot(rng, bits, n_chrom, 8)
        fixed += [tuple(int(x) for x in row) for row in crafted[:4]]
        spare = crafted[4:]
    fixed = np.array(fixed[:V], dtype=np.int64)
    taken = set((int(c), int(p)) for c, p, _b in fixed) | set((int(c), int(p)) for c, p, _b in spare)
    n_sites = V + 8
    chrom = rng.integers(0, n_chrom, n_sites)
    near = rng.random(n_sites) < 0.5   # half of the sites next to each other, half anywhere in int32
    pos = np.where(near, rng.integers(0, 8 * V + 16, n_sites), rng.integers(0, POS_MAX, n_sites))
    _, first = np.unique(chrom << 31 | pos, return_index=True)
    first = np.array([i for i in np.sort(first) if (int(chrom[i]), int(pos[i])) not in taken], dtype=np.int64)
    chrom, pos = chrom[first], pos[first]
    n_alleles = rng.choice([1, 1, 2, 3, 5], size=len(first))
    rank = np.argsort(rng.random((len(first), 5)), axis=1)   # rank[s, b] < n_alleles[s]: base b is an allele of site s
    site, base = np.nonzero(rank < n_alleles[:, None])
    rows = np.concatenate([fixed, np.stack([chrom[site], pos[site], base], axis=1)])[:V]
    assert len(rows) == V and len(np.unique(variant_key(rows[:, 0], rows[:, 1], rows[:, 2]))) == V
    perm = rng.permutation(V)   # rows in any order: var_chrom is not sorted
    rows = rows[perm]
    where = np.empty(V, dtype=np.int64)
    where[perm] = np.arange(V)
    _, v2snp = np.unique(rows[:, 0] << 31 | rows[:, 1], return_inverse=True)
    return rows, v2snp.astype(np.int32), where[:len(fixed)], spare


def _run_members(rng, case, m):
    """The p_base_wrong members of every run of equal (variant, barcode), the runs that must come first listed first."""
    mode = case.get('runs', 'mixed')
    if mode == 'one':
        return [(0.99 + 0.01 * rng.random(m)).astype(np.float32)] if m else []
    if mode == 'unique':
        return [np.array([x], dtype=np.float32) for x in (0.5 + 0.5 * rng.random(m)).astype(np.float32)]
    plain = lambda k: (0.5 + 0.5 * rng.random(k)).astype(np.float32)  # noqa: E731
    u = lambda: np.float32(1 + rng.random())  # noqa: E731
    planned = [plain(3), plain(2)]   # the first and the last run of the sorted calls: several members each
    planned += [plain(2) for _ in range(6)]   # the runs on the keys that the calls must reach
    if case.get('long'):
        planned.append((0.99 + 0.01 * rng.random(5000)).astype(np.float32))
    if case.get('float_edges'):
        for _ in range(30):   # subnormal products, whatever the order
            planned.append(np.array([np.float32(1e-19) * u(), np.float32(1e-20) * u(), 0.1 + 0.9 * rng.random()], dtype=np.float32))
        for _ in range(6):    # products that underflow to exactly 0
            planned.append(np.array([np.float32(1e-30) * u(), np.float32(1e-30) * u()], dtype=np.float32))
        x, y = plain(2)
        planned += [np.array(a, dtype=np.float32) for a in ([1, x, 1], [x, 0, y], [1e-38, x], [x, 1e-38, y, 1], [1e-38], [0], [1])]
    runs, budget = [], m
    for members in planned:
        if len(members) <= budget:
            runs.append(members)
            budget -= len(members)
    lengths = rng.choice(RUN_LENGTHS, size=budget, p=[.45, .2, .15, .12, .08])
    lengths = lengths[np.cumsum(lengths) <= budget]
    rest = budget - int(lengths.sum())
    for k in list(lengths) + ([rest] if rest else []):
        runs.append(plain(int(k)))
    return runs


def _container(rng, cb, pos, base, p, n_barcodes, with_spare_molecules=True):
    """CompressedSNPCalls of these calls: molecules of up to three calls of a barcode each, unused molecules among them,
    in shuffled molecule order."""
    from demuxalot_amd import CompressedSNPCalls
    n = len(cb)
    order = np.argsort(cb, kind='stable')
    s_cb = cb[order]
    head = np.concatenate([[True], s_cb[1:] != s_cb[:-1]]) if n else np.zeros(0, dtype=bool)
    group = np.cumsum(head) - 1
    rank = np.arange(n) - np.flatnonzero(head)[group] if n else np.zeros(0, dtype=np.int64)
    _, first, inverse = np.unique(group * (n + 1) + rank // 3, return_index=True, return_inverse=True)
    n_used = len(first)
    n_spare = (n_used // 4 + 2) if with_spare_molecules else 0
    new_id = rng.permutation(n_used + n_spare)
    mol_cb = np.empty(n_used + n_spare, dtype=np.int32)
    mol_cb[new_id[:n_used]] = s_cb[first]
    mol_cb[new_id[n_used:]] = rng.integers(0, n_barcodes, n_spare)
    call_mol = np.empty(n, dtype=np.int32)
    call_mol[order] = new_id[inverse.reshape(-1)] if n else []
    return CompressedSNPCalls.from_arrays(mol_cb, call_mol, pos, base, p)


def make(case):
    rng = np.random.default_rng(case['seed'])
    V, n, B = case['V'], case['n_calls'], case['n_barcodes']
    n_chrom = min(3, V)
    rows, v2snp, must_reach, spare_keys = _variants(rng, V, n_chrom)
    m = min(n, case.get('n_matched', int(round(0.7 * n))))
    silent = (np.arange(B) % 5 == 2) & (np.arange(B) > 0) & (np.arange(B) < B - 1)   # barcodes without calls
    allowed = np.flatnonzero(~silent)

    # matched calls: runs of equal (variant, barcode)
    runs = _run_members(rng, case, m)
    R = len(runs)
    forced = []
    if case.get('runs', 'mixed') == 'mixed':
        reach = [r for i, r in enumerate(must_reach) if i < 2 or i >= 6]   # positions 2^31 - 1 and 0, the last slot's variants
        forced = [(0, 0), (V - 1, B - 1)] + [(int(r), int(rng.choice(allowed))) for r in reach]
        forced = list(dict.fromkeys(forced))[:R]
    elif case['runs'] == 'one':
        forced = [(int(must_reach[0]), B - 1)][:R]   # on the chromosome that is split over two containers
    n_pairs = V * len(allowed)
    if R > n_pairs:   # fewer pairs than runs: the last pair takes the rest
        runs = runs[:n_pairs - 1] + [np.concatenate(runs[n_pairs - 1:])]
        R = n_pairs
    pid = rng.choice(n_pairs, size=min(n_pairs, R + len(forced)), replace=False)
    pairs = [(int(q) // len(allowed), int(allowed[int(q) % len(allowed)])) for q in pid]
    is_forced = set(forced)
    pairs = (forced + [pr for pr in pairs if pr not in is_forced])[:R]
    assert len(pairs) == R and len(set(pairs)) == R
    lengths = np.array([len(r) for r in runs], dtype=np.int64)
    mv = np.repeat(np.array([pr[0] for pr in pairs], dtype=np.int64), lengths)
    mcb = np.repeat(np.array([pr[1] for pr in pairs], dtype=np.int64), lengths)
    mp = np.concatenate(runs) if runs else np.zeros(0, dtype=np.float32)
    assert len(mv) == m

    # unmatched calls: a variant's position with another base, a position without variants, keys of the last table slot
    k = n - m
    site_bases = np.bincount(v2snp, weights=1 << rows[:, 2], minlength=1).astype(np.int64)   # bit b: base b is an allele
    open_rows = np.flatnonzero(site_bases[v2snp] != 31)
    kind = rng.integers(0, 2, k) if len(open_rows) else np.ones(k, dtype=np.int64)
    at = open_rows[rng.integers(0, len(open_rows), k)] if len(open_rows) else np.zeros(k, dtype=np.int64)
    other = rng.integers(0, 5, k)
    for _ in range(5):
        other = np.where(site_bases[v2snp[at]] >> other & 1, (other + 1) % 5, other)
    u_chrom = np.where(kind == 0, rows[at, 0], rng.integers(0, n_chrom, k))
    u_pos = np.where(kind == 0, rows[at, 1], np.where(rng.random(k) < 0.5, rng.integers(0, 8 * V + 16, k), rng.integers(0, POS_MAX, k)))
    u_base = np.where(kind == 0, other, rng.integers(0, 5, k))
    sites = np.unique(rows[:, 0] << 31 | rows[:, 1])
    for _ in range(64):
        on_site = (kind == 1) & np.isin(u_chrom << 31 | u_pos, sites)
        if not on_site.any():
            break
        u_pos = np.where(on_site, (u_pos + 12345) % POS_MAX, u_pos)
    assert not ((kind == 1) & np.isin(u_chrom << 31 | u_pos, sites)).any()
    n_spare = min(k // 8, 3 * len(spare_keys))   # a few calls on every spare key of the last slot
    for j in range(n_spare):
        u_chrom[j], u_pos[j], u_base[j] = spare_keys[j % len(spare_keys)]
    u_cb = allowed[rng.integers(0, len(allowed), k)]
    u_p = rng.choice([0.0, 1e-38, 0.02, 1.0], size=k).astype(np.float32)

    chrom = np.concatenate([rows[mv, 0], u_chrom]).astype(np.int32)
    pos = np.concatenate([rows[mv, 1], u_pos]).astype(np.int32)
    base = np.concatenate([rows[mv, 2], u_base]).astype(np.uint8)
    cb = np.concatenate([mcb, u_cb]).astype(np.int32)
    p = np.concatenate([mp, u_p]).astype(np.float32)

    # containers: the last chromosome first and split over two containers, the others in descending order, an empty
    # container on a chromosome without variants and one on a chromosome with variants among them
    split = n_chrom - 1
    layout = [split, -1] + list(range(n_chrom - 2, -1, -1)) + [split, 0]   # chromosome of every container
    part = np.array([layout.index(c) if c != split else 0 for c in range(n_chrom)], dtype=np.int64)[chrom]
    second = len(layout) - 2
    part[(chrom == split) & (rng.random(n) < 0.5)] = second
    order = np.lexsort((rng.random(n), part))   # container after container, the calls of each in shuffled order
    chrom, pos, base, cb, p, part = (a[order] for a in (chrom, pos, base, cb, p, part))
    containers = []
    for j, c in enumerate(layout):
        sel = part == j
        containers.append((c, _container(rng, cb[sel], pos[sel], base[sel], p[sel], B, with_spare_molecules=c >= 0)))
    return types.SimpleNamespace(
        var_chrom=rows[:, 0].astype(np.int32), var_pos=rows[:, 1].astype(np.int32), var_base=rows[:, 2].astype(np.uint8), v2snp=v2snp,
        chrom=chrom, pos=pos, base=base, cb=cb, p=p, containers=containers, n_barcodes=B, n_variants=V, n_calls=n)


@functools.lru_cache(maxsize=None)
def problem(name):
    return make(CASES[name])


def container_list(prob, provisional=False):
    """The containers as DeviceContext.pack_containers_and_set_problem takes them (chromosome numbers of var_chrom), or
    as DeviceContext.stage_containers does (provisional: the position in the list)."""
    return [(k if provisional else chrom, c.snp_calls[:c.n_snp_calls], c.molecules[:c.n_molecules])
            for k, (chrom, c) in enumerate(prob.containers)]


def chrom_of_container(prob):
    return [chrom for chrom, _c in prob.containers]


def with_barcode(prob, call, value):
    """A copy of the problem in which molecule call `call` (index into the flat arrays) sits on barcode `value`: in the
    containers through a molecule of its own."""
    import copy
    out = copy.copy(prob)
    out.cb = prob.cb.copy()
    out.cb[call] = value
    out.containers = list(prob.containers)
    at = call
    for j, (chrom, c) in enumerate(prob.containers):
        if at < c.n_snp_calls:
            from demuxalot_amd import CompressedSNPCalls
            calls, molecules = c.snp_calls[:c.n_snp_calls], c.molecules[:c.n_molecules]
            call_mol = calls['molecule_index'].copy()
            call_mol[at] = len(molecules)
            out.containers[j] = (chrom, CompressedSNPCalls.from_arrays(
                np.concatenate([molecules['compressed_cb'], [value]]), call_mol, calls['snp_position'], calls['base_index'], calls['p_base_wrong']))
            return out
        at -= c.n_snp_calls
    raise IndexError(call)


# ---- expected values ----------------------------------------------------------------------------------------------------
def flat_from_containers(prob):
    """The flat call arrays read back from the containers the way the reference flattens them (demux.py:332-358)."""
    parts = [(chrom, c.snp_calls[:c.n_snp_calls], c.molecules[:c.n_molecules]) for chrom, c in prob.containers]
    cat = lambda arrays, dtype: np.concatenate([np.asarray(a, dtype=dtype) for a in arrays])  # noqa: E731
    return (cat([np.full(len(c), chrom) for chrom, c, _m in parts], np.int32), cat([c['snp_position'] for _k, c, _m in parts], np.int32),
            cat([c['base_index'] for _k, c, _m in parts], np.uint8),
            cat([m['compressed_cb'][c['molecule_index']] if len(c) else [] for _k, c, m in parts], np.int32),
            cat([c['p_base_wrong'] for _k, c, _m in parts], np.float32))


def expected(prob, oracle):
    """What the reference's pack gives: per-call variant, n_matched, n_unique, the unique (variant, cb, p, count),
    mol_per_variant, and the matched molecule calls themselves."""
    lookup = {key: i for i, key in enumerate(zip(prob.var_chrom.tolist(), prob.var_pos.tolist(), prob.var_base.tolist()))}
    assert len(lookup) == prob.n_variants
    call_variant = np.array([lookup.get(key, -1) for key in zip(prob.chrom.tolist(), prob.pos.tolist(), prob.base.tolist())],
                            dtype=np.int32).reshape(prob.n_calls)
    keep = call_variant != -1
    mol_v, mol_cb, mol_p = call_variant[keep], prob.cb[keep], prob.p[keep]
    variant, cb, p, count = oracle.dedupe_calls(mol_v, mol_cb, mol_p)
    return types.SimpleNamespace(call_variant=call_variant, n_matched=int(keep.sum()), n_unique=len(variant), variant=variant, cb=cb, p=p,
                                 count=count, mol_per_variant=np.bincount(mol_v, minlength=prob.n_variants).astype(np.int64),
                                 mol_variant=mol_v, mol_cb=mol_cb, mol_p=mol_p)


@functools.lru_cache(maxsize=None)
def _expected_of(name, oracle):
    return expected(problem(name), oracle)


def expected_of(name, oracle):
    """expected(problem(name), oracle), computed once per case; nobody writes to it."""
    return _expected_of(name, oracle)


# ---- which cases a problem holds ----------------------------------------------------------------------------------------
def cases_hit(prob, want, oracle):
    hit = collections.Counter()
    V, B, n, m = prob.n_variants, prob.n_barcodes, prob.n_calls, want.n_matched
    hit[f'n_calls={n}'] = hit[f'matched={m}' + (' of some' if n and not m else '')] = hit[f'V={V}'] = hit[f'n_barcodes={B}'] = 1
    # sizes
    hit['calls on the last barcode'] = int((want.cb == B - 1).sum())
    hit['barcodes without calls'] = B - len(np.unique(prob.cb)) if n else 0
    # runs, from the oracle's unique calls (variant-major, the sorted order) and the matched calls in call order
    key = want.mol_variant.astype(np.int64) << 32 | want.mol_cb
    order = np.argsort(key, kind='stable')
    start = np.cumsum(want.count) - want.count
    for length in RUN_LENGTHS + (5000,):
        hit[f'run of {length}'] = int((want.count == length).sum())
    if m:
        backwards = oracle.dedupe_calls(want.mol_variant[::-1], want.mol_cb[::-1], want.mol_p[::-1])[2]
        hit['product depends on the order'] = int((backwards.view(np.uint32) != want.p.view(np.uint32)).sum())
        spread = np.maximum.reduceat(order, start) - np.minimum.reduceat(order, start) + 1
        hit['run scattered through the call order'] = int(((want.count > 1) & (spread > want.count)).sum())
        hit['run from the last 10 slots of a block into the next'] = int(((start % 256 >= 246) & (start % 256 + want.count > 256)).sum())
        hit['first run has several members'] = int(want.count[0] > 1)
        hit['last run has several members'] = int(want.count[-1] > 1)
        hit['every call in one run'] = int(want.n_unique == 1 and m == n and n > 256)
        hit['every call unique'] = int(want.n_unique == m == n and n > 256)
        smallest = np.minimum.reduceat(want.mol_p[order], start)
        hit['subnormal product'] = int(((want.p > 0) & (want.p < TINY)).sum())
        hit['product underflows to 0'] = int(((want.p == 0) & (smallest > 0) & (want.count > 1)).sum())
        for value, name in ((0.0, '0'), (1.0, '1'), (1e-38, '1e-38')):
            hit[f'member {name}'] = int((want.mol_p == np.float32(value)).sum())
    # matching
    sites, alleles = np.unique(prob.var_chrom.astype(np.int64) << 31 | prob.var_pos, return_counts=True)
    hit['site with the bases 0..4'] = int((alleles == 5).sum())
    on_site = np.isin(prob.chrom.astype(np.int64) << 31 | prob.pos, sites)
    listed = np.isin(prob.chrom, prob.var_chrom)
    hit['call at a variant position with another base'] = int((on_site & (want.call_variant < 0)).sum())
    hit['call on a listed chromosome at a position without variants'] = int((listed & ~on_site).sum())
    for position, name in ((0, '0'), (POS_MAX, '2^31 - 1')):
        hit[f'matched call at position {name}'] = int(((prob.pos == position) & (want.call_variant >= 0)).sum())
    hit['var_chrom not sorted'] = int((np.diff(prob.var_chrom) < 0).any())
    hit['three chromosomes'] = int(len(np.unique(prob.var_chrom)) == 3)
    hit['about 30 % unmatched'] = int(n > 0 and 0.25 <= 1 - m / n <= 0.35)
    bits = table_bits(V)
    last = np.uint64((1 << bits) - 1)
    hit['variant in the last table slot'] = int((slot_of(variant_key(prob.var_chrom, prob.var_pos, prob.var_base), bits) == last).sum())
    call_slot = slot_of(variant_key(prob.chrom, prob.pos, prob.base), bits)
    hit['matched call on a variant of the last table slot'] = int(((call_slot == last) & (want.call_variant >= 0)).sum())
    hit['unmatched call in the last table slot'] = int(((call_slot == last) & (want.call_variant < 0)).sum())
    hit['table of 64 slots'] = int(bits == 6)
    hit['table half full'] = int(V + 1 == 1 << (bits - 1))
    # containers
    sizes = [(chrom, c.n_snp_calls, c.n_molecules) for chrom, c in prob.containers]
    with_variants = set(prob.var_chrom.tolist())
    hit['container with 0 calls'] = sum(1 for chrom, calls, _m in sizes if calls == 0 and chrom in with_variants)
    hit['empty container on a chromosome without variants'] = sum(1 for chrom, calls, _m in sizes if calls == 0 and chrom not in with_variants)
    filled = collections.Counter(chrom for chrom, calls, _m in sizes if calls > 0)
    hit['chromosome split over two containers'] = sum(1 for count in filled.values() if count == 2)
    table = chrom_of_container(prob)
    hit['container order differs from the numbering'] = int(any(calls > 0 and chrom != k for k, (chrom, calls, _m) in enumerate(sizes))
                                                            and table != sorted(table))
    used = [len(np.unique(c.snp_calls['molecule_index'][:c.n_snp_calls])) for _chrom, c in prob.containers]
    hit['molecule table larger than the calls use'] = sum(1 for (_c, calls, mols), u in zip(sizes, used) if calls and mols > u)
    hit['molecule with several calls'] = sum(int((np.bincount(c.snp_calls['molecule_index'][:c.n_snp_calls]) > 1).sum())
                                             for _chrom, c in prob.containers if c.n_snp_calls)
    return +hit   # (without the zero entries)
