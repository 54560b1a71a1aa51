// The E-step's policy (demuxalot_amd/csrc/estep_plan.h) over the cross product of its fact space, on the CPU: the sequence run_estep makes
// of the plan's stages is replayed on plain values, the invariants every combination must keep are asserted, then the named rows of the
// decision table in DESIGN.md 4.1 one by one.  Built with -fsanitize=address,undefined and run by tests/test_estep_plan_cpu.py; prints
// the number of combinations walked.
#include <cstdio>
#include <initializer_list>

#include "estep_plan.h"

using namespace dmx::eplan;

namespace {  // (the header's types are hidden: everything here is this program's own)

static long long failures = 0;
static Facts failed;
static void report(const char *what, int line)
{
    const Facts &f = failed;
    if (failures++ < 20)
        std::fprintf(stderr,
                     "line %d: %s\n  mode %d doublets %d prior %d kept %d G %d K %d B %lld rows %lld | schedule %d bins %lld stream %d coarse_ready %d coarse_pass %d "
                     "adaptive %d lean %d lo %g | prob16 %d sliced %d lists %d | dict %d candidate %d call_rows %d below4g %d | packing %d stat %d long %lld %lld %lld | "
                     "segments %d pair_blocks %d\n",
                     line, what, (int)f.mode, f.with_doublets, f.with_prior, f.logits_kept, f.G, f.K, f.B, f.table_rows, f.schedule, f.n_bins, f.tile_stream,
                     f.coarse_ready, f.coarse_pass, f.guard_adaptive, f.lean_memory, (double)f.lo, f.prob16_valid, f.sliced, f.table_lists, f.dict_mode,
                     f.dict_candidate, f.call_rows, f.records_below_4g, f.packing, f.row_statistic, f.n_long_rows[0], f.n_long_rows[1], f.n_long_rows[2],
                     f.segments, f.n_pair_blocks);
}
#define CHECK(cond) ((cond) ? (void)0 : (failed = f, report(#cond, __LINE__)))
#define IMPLIES(a, b) CHECK(!(a) || (b))

// one E-step as run_estep sequences it: what ran, and the facts it leaves
enum Branch { BR_DICT_LANE, BR_DICT_BLOCK, BR_PACKED, BR_GUARDED, BR_PLAIN };
struct Ran {
    Branch branch;
    bool fast;           // the arithmetic of the main launch
    Kernel coarse;       // guarded with the coarse level offered (else kind = KERNEL_REFUSED and not counted)
    bool coarse_issued;
    Kernel main;         // the fine level / the only launch
    Kernel redo;         // guarded
    Walk walk;
    bool built, released, converted;
    Facts after;
};
// a launch's request as launch_estep gets it: through the arrays run_estep attaches (handover) and the read-back (request_of)
static Request request(const Facts &f, bool fast, Walk w, bool coarse, bool listed)
{
    const Handover h = handover(w, coarse);
    const Request r = request_of(f.K, f.with_doublets && !coarse, fast, f.schedule, h.bins ? bins(f) : 0, h.prob16, h.coarse_records, segments_offered(f), listed, f.n_pair_blocks);
    // the pair is lossless wherever there are bins to walk (without bins every walk is a barcode per wavefront)
    if (bins(f) > 0 && (r.walk != w || r.coarse != coarse)) failed = f, report("request_of(handover(walk, coarse)) == (walk, coarse)", __LINE__);
    return r;
}
static inline Ran estep(Facts f, unsigned distinct)
{
    Ran r{};
    if (unused_stream_release_due(f)) f.tile_stream = false;
    r.fast = tolerance_arithmetic(f);
    DictForm d = DICT_NONE;
    if (!coarse_first(f) && dictionary_admissible(f)) d = dictionary_form(f, distinct, 64);
    const Packed p = packed_candidate(f);
    if (d != DICT_NONE) {
        r.branch = d == DICT_LANE ? BR_DICT_LANE : BR_DICT_BLOCK;
    } else if (packed_runs(f, p)) {
        r.branch = BR_PACKED;
        r.fast = false;
    } else if (guarded(f)) {
        r.branch = BR_GUARDED;
        r.built = coarse_build_due(f), r.released = lean_release_due(f);
        r.coarse_issued = allow_coarse(f);
        r.converted = prob16_conversion_due(f);
        if (r.built) f.coarse_ready = true;
        if (r.released) f.tile_stream = f.call_rows = false;
        if (r.converted) f.prob16_valid = prob16_stays_valid(f);
        if (r.coarse_issued) r.coarse = kernel(request(f, true, WALK_COARSE_RECORDS, true, false));
        r.walk = walk(f);
        r.main = kernel(request(f, true, r.walk, false, false));
        r.redo = kernel(request(f, false, WALK_BARCODE_MAJOR, false, true));
    } else {
        r.branch = BR_PLAIN;
        r.walk = walk(f);
        r.main = kernel(request(f, r.fast, r.walk, false, false));
    }
    r.after = f;
    return r;
}

static inline bool tiled_kind(KernelKind k) { return k == KERNEL_TILED || k == KERNEL_TILED_TWO_CALLS || k == KERNEL_COARSE || k == KERNEL_FINE8; }

static inline void invariants(const Facts f, unsigned distinct)
{
    const Ran r = estep(f, distinct);
    const bool admitted = f.G <= 1024;  // ensure_options
    const bool launches = r.branch == BR_GUARDED || r.branch == BR_PLAIN;
    // every admitted combination gets exactly one form, and each of its launches a kernel; singlets beyond 1024 are refused
    if (launches) {
        IMPLIES(admitted, r.main.kind != KERNEL_REFUSED);
        IMPLIES(!f.with_doublets && f.K > 1024, r.main.kind == KERNEL_REFUSED);
        IMPLIES(r.main.kind == KERNEL_REFUSED, !f.with_doublets && f.K > 1024);
    }
    if (r.branch == BR_GUARDED) {
        IMPLIES(admitted, r.redo.kind != KERNEL_REFUSED && !r.redo.fast);
        CHECK(r.redo.kind == KERNEL_DIRECT || r.redo.kind == KERNEL_BLOCK_TILES || r.redo.kind == KERNEL_REFUSED);  // listed barcodes: neither split nor pair blocks nor tiles
        IMPLIES(r.coarse_issued, r.coarse.kind == KERNEL_COARSE && r.coarse.cpg == coarse_calls_per_gather(f.K));
        CHECK(r.main.fast);
    }
    // the coarse pass: only guarded, singlets of the tile shape on a built schedule, a clip that keeps binary16 normal, nobody reading the logits
    // unless dmx_set_coarse_pass(2)
    const bool coarse_ran = r.branch == BR_GUARDED && r.coarse_issued;
    IMPLIES(coarse_ran, f.mode == MODE_GUARDED && !f.with_doublets && f.K >= 17 && f.K <= 128 && f.schedule != 0 && f.n_bins > 0 && f.lo >= 6.2e-5f &&
                            f.coarse_pass != 0 && (!f.logits_kept || f.coarse_pass == 2) && r.after.coarse_ready);
    IMPLIES(r.branch != BR_GUARDED, !r.built && !r.released && !r.converted);
    IMPLIES(r.built, coarse_ran && f.tile_stream && !f.coarse_ready);
    IMPLIES(r.released, r.built && f.lean_memory && !r.after.tile_stream && !r.after.call_rows);
    IMPLIES(r.converted, coarse_ran && !f.prob16_valid);
    IMPLIES(coarse_ran, r.converted || f.prob16_valid);
    // fine8 only without the tile stream and with the coarse records; a barcode-major walk never a tiled kernel
    if (launches) {
        IMPLIES(r.main.kind == KERNEL_FINE8, !r.after.tile_stream && r.after.coarse_ready && r.walk == WALK_COARSE_RECORDS && r.main.fast);
        IMPLIES(r.walk == WALK_BARCODE_MAJOR, !tiled_kind(r.main.kind));
        IMPLIES(tiled_kind(r.main.kind), singlet_tile_shape(f.K, f.with_doublets) && f.schedule != 0 && f.n_bins > 0);
        IMPLIES(r.main.kind == KERNEL_TILED && !r.main.fast, f.schedule == 2 && f.K > 32 && r.after.tile_stream);
        IMPLIES(r.walk == WALK_TILE_STREAM, r.after.tile_stream);
        IMPLIES(r.main.kind == KERNEL_COARSE, false);  // the coarse level is a launch of its own
        IMPLIES(r.main.kind == KERNEL_DIRECT_SPLIT, r.main.fast && r.main.L == 64 && f.segments && f.K <= 1024);
        IMPLIES(r.main.kind == KERNEL_PAIR_BLOCKS, r.main.fast && f.with_doublets && f.n_pair_blocks > 0 && (r.main.threads == 512) == (f.n_pair_blocks >= 1024));
        IMPLIES(r.main.kind == KERNEL_DIRECT || r.main.kind == KERNEL_DIRECT_SPLIT, r.main.L * r.main.A >= f.K && r.main.L * r.main.A < 2 * (f.K < 4 ? 4 : f.K));
        IMPLIES(r.main.kind == KERNEL_BLOCK_TILES, r.main.tile * 256 * r.main.launches >= f.K && r.main.tile <= 17 && (!r.main.fast || r.main.tile <= 6));
    }
    // a guarded E-step with a prior on a workgroup-per-barcode shape runs exact; the two stages' shapes agree.  The thresholds are written
    // out here, not taken from the header: option tables beyond 1024; doublet tables beyond 512, beyond 256 with the tolerance arithmetic
    const bool wide_for_tolerance = f.K > 1024 || (f.with_doublets && f.K > 256), wide_for_exact = f.K > 1024 || (f.with_doublets && f.K > 512);
    CHECK(block_shape(f.K, f.with_doublets, true) == wide_for_tolerance && block_shape(f.K, f.with_doublets, false) == wide_for_exact);
    CHECK(tolerance_arithmetic(f) == (f.mode == MODE_FAST || (f.mode == MODE_GUARDED && !(f.with_prior && wide_for_tolerance))));
    if (launches) {
        const bool block_kernel = r.main.kind == KERNEL_BLOCK_TILES || r.main.kind == KERNEL_PAIR_BLOCKS;
        IMPLIES(r.main.kind != KERNEL_REFUSED, block_kernel == (r.main.fast ? wide_for_tolerance : wide_for_exact));
        IMPLIES(tiled_kind(r.main.kind), !f.with_doublets && f.K >= 17 && f.K <= 128);
        IMPLIES(r.main.kind == KERNEL_TILED_TWO_CALLS, f.K <= 32);
        IMPLIES(r.main.kind == KERNEL_DIRECT || r.main.kind == KERNEL_DIRECT_SPLIT, f.K <= 1024 && r.main.L == (f.K <= 4 ? 4 : f.K <= 8 ? 8 : f.K <= 16 ? 16 : f.K <= 32 ? 32 : 64));
    }
    if (r.branch == BR_GUARDED) IMPLIES(r.redo.kind == KERNEL_BLOCK_TILES, wide_for_exact);
    IMPLIES(f.mode == MODE_GUARDED && f.with_prior && block_shape(f.K, f.with_doublets, true), r.branch != BR_GUARDED && !r.fast);
    IMPLIES(f.mode == MODE_EXACT, !r.fast && r.branch != BR_GUARDED);
    // packed: never with the tolerance arithmetic, only doublets of a packed shape
    IMPLIES(r.branch == BR_PACKED, !r.fast && f.with_doublets && f.mode != MODE_FAST && f.packing != 0 && f.records_below_4g && f.K <= 160);
    // a dictionary form: call_rows present, not the fast mode, not ahead of a coarse pass nobody reads
    IMPLIES(r.branch == BR_DICT_LANE || r.branch == BR_DICT_BLOCK, f.call_rows && f.mode != MODE_FAST && f.dict_mode != 0 && f.B > 0 && f.table_rows > 0 &&
                                                                      distinct >= 1 && distinct <= (f.with_doublets ? 4u : 8u));
    IMPLIES(r.branch == BR_DICT_LANE, f.K <= 256 && f.records_below_4g);
    IMPLIES(r.branch == BR_DICT_BLOCK, f.with_doublets && f.K > 256);
    IMPLIES(f.dict_mode == 0, r.branch != BR_DICT_LANE && r.branch != BR_DICT_BLOCK);
    // behind a lean-memory release the refreshed facts walk what the released state walks at the next E-step
    if (r.released) {
        Facts next = r.after;
        next.logits_kept = false;
        const Ran n = estep(next, 0);
        CHECK(n.branch == BR_GUARDED && n.walk == r.walk && n.main.kind == r.main.kind && !n.built && !n.released);
        CHECK(r.walk == WALK_COARSE_RECORDS && r.main.kind == KERNEL_FINE8);
    }
    // coarse_capable is one definition: what the P-step's caller asked of the table ahead holds for run_estep behind it
    IMPLIES(coarse_ran, coarse_capable(f, f.lo));
}

struct Shape {
    int G;
    bool doublets;
};
// singlets on either side of every threshold; doublet tables K = G (G + 1) / 2 = 3, 6, 10, 15, 21, 28, 36, 55, 66, 120, 136, 253, 276, 496, 528, 990, 1035, 8256
static const Shape SHAPES[] = {{4, false},   {5, false},   {8, false},   {9, false},   {16, false},   {17, false},  {32, false}, {33, false}, {64, false},
                               {65, false},  {128, false}, {129, false}, {256, false}, {257, false},  {512, false}, {513, false}, {1024, false}, {1025, false},
                               {2, true},    {3, true},    {4, true},    {5, true},    {6, true},     {7, true},    {8, true},   {10, true},  {11, true},
                               {15, true},   {16, true},   {22, true},   {23, true},   {31, true},    {32, true},   {44, true},  {45, true},  {128, true}};
static int pair_blocks_of(int G)  // ensure_options: 2 x 3 blocks of the triangle
{
    int n = 0;
    for (int i = 0; 2 * i < G; i++)
        for (int j = 0; 3 * j < G; j++) n += 3 * j + 2 >= 2 * i;
    return n;
}

static long long walk_all()
{
    long long n = 0;
    Facts f{};
    const unsigned distincts[] = {0, 3, 4, 5, 8, 9};
    for (const Shape &sh : SHAPES)
        for (int mode = 0; mode < 3; mode++)
            for (int pk = 0; pk < 4; pk++)  // with_prior x logits_kept
                for (long long B : {0ll, 8192ll})
                    for (long long rows : {0ll, 100000ll, 1ll << 24})
                        for (int sched = 0; sched < 6; sched++)  // schedule x bins
                            for (int st = 0; st < 4; st++)       // tile_stream x coarse_ready
                                for (int cp = 0; cp < 24; cp++)  // coarse_pass x guard_adaptive x lean_memory x lo
                                    for (int dict = 0; dict < 7; dict++)
                                        for (int below = 0; below < 2; below++)
                                            for (int pack = 0; pack < 7; pack++) {
                                                f.G = sh.G, f.with_doublets = sh.doublets, f.K = sh.doublets ? sh.G * (sh.G + 1) / 2 : sh.G;
                                                f.mode = (Mode)mode, f.with_prior = (pk & 1) != 0, f.logits_kept = (pk & 2) != 0;
                                                f.B = B, f.table_rows = rows;
                                                f.schedule = sched / 2, f.n_bins = sched & 1 ? 50 : 0;
                                                f.tile_stream = (st & 1) != 0, f.coarse_ready = (st & 2) != 0;
                                                f.coarse_pass = cp % 3, f.guard_adaptive = (cp / 3 & 1) != 0, f.lean_memory = (cp / 6 & 1) != 0;
                                                f.lo = cp / 12 ? 6.2e-5f : 6.1e-5f;
                                                // never; where it pays x (candidate, call_rows); wherever it exists x call_rows
                                                f.dict_mode = dict == 0 ? 0 : dict <= 4 ? 1 : 2;
                                                f.dict_candidate = dict <= 4 ? ((dict - 1) & 1) != 0 : true, f.call_rows = dict <= 4 ? ((dict - 1) & 2) != 0 : dict == 6;
                                                f.records_below_4g = below != 0;
                                                // never; where it pays x (no statistic, no long rows, an eighth, one more); every barcode; the split wherever
                                                f.packing = pack == 0 ? 0 : pack <= 4 ? 1 : pack == 5 ? 2 : 3;
                                                f.row_statistic = pack != 1;
                                                const long long nl = pack == 3 ? B / 8 : pack == 4 || pack == 6 ? B / 8 + 1 : 0;
                                                f.n_long_rows[0] = f.n_long_rows[1] = f.n_long_rows[2] = nl;
                                                // the facts that feed one predicate each cycle along the walk instead of multiplying it (and `distinct` behind them: every pair of the two)
                                                const int leaf = (int)(n % 32);
                                                f.prob16_valid = (leaf & 1) != 0, f.sliced = (leaf & 2) != 0, f.table_lists = (leaf & 4) != 0, f.segments = (leaf & 8) != 0;
                                                f.n_pair_blocks = sh.doublets && f.K > 256 && !(leaf & 16) ? pair_blocks_of(sh.G) : 0;
                                                invariants(f, distincts[n / 32 % 6]);
                                                n++;
                                            }
    return n;
}

// the flagship: 200k barcodes x 100k SNPs x 64 genotypes, singlets, the library's defaults, an E-step inside a dmx_em call
static Facts flagship()
{
    Facts f{};
    f.mode = MODE_GUARDED, f.G = f.K = 64, f.B = 200000, f.table_rows = 100000;
    f.schedule = 1, f.n_bins = 25000, f.tile_stream = true, f.coarse_pass = 1, f.guard_adaptive = true, f.lo = 1e-4f;
    f.dict_mode = 1, f.call_rows = true, f.records_below_4g = true, f.packing = 1, f.row_statistic = true;
    return f;
}
static Facts doublets_of(int G, long long B)
{
    Facts f = flagship();
    f.with_doublets = true, f.G = G, f.K = G * (G + 1) / 2, f.B = B, f.n_long_rows[0] = f.n_long_rows[1] = f.n_long_rows[2] = B / 100;
    f.n_pair_blocks = f.K > 256 ? pair_blocks_of(G) : 0;
    return f;
}

static void table_rows()
{
    {  // "first of a call": table without addition, nobody reads the logits: the coarse pass comes first, the dictionary is not tried; records built
        Facts f = flagship();
        f.dict_candidate = true;
        CHECK(coarse_capable(f, f.lo) && coarse_first(f));
        const Ran r = estep(f, 3);
        CHECK(r.branch == BR_GUARDED && r.built && !r.released && r.converted && r.coarse.kind == KERNEL_COARSE && r.coarse.cpg == 2);
        CHECK(r.main.kind == KERNEL_TILED && r.main.A == 1 && r.main.fast && r.redo.kind == KERNEL_DIRECT && r.redo.L == 64 && r.redo.A == 1 && r.redo.U == 8);
    }
    {  // "predict": the same table, logits kept: the dictionary's lane form (200k x 16 / 64 lanes >= 8192)
        Facts f = flagship();
        f.dict_candidate = f.logits_kept = true;
        CHECK(!coarse_first(f) && dictionary_admissible(f));
        CHECK(estep(f, 3).branch == BR_DICT_LANE && estep(f, 9).branch == BR_GUARDED && !estep(f, 9).coarse_issued);
        f.B = 20000;  // one round of wavefronts: the lane form does not pay
        CHECK(!dictionary_admissible(f));
        f.dict_mode = 2;
        CHECK(dictionary_admissible(f));
    }
    {  // "steady state": iterations 1.. of a call, P-step wrote the binary16 table: coarse + fine + redo, nothing built or converted
        Facts f = flagship();
        f.coarse_ready = f.prob16_valid = true;
        const Ran r = estep(f, 0);
        CHECK(r.branch == BR_GUARDED && r.coarse_issued && !r.built && !r.converted && r.main.kind == KERNEL_TILED && r.walk == WALK_TILE_STREAM);
        f.logits_kept = true;  // "last of a call": no coarse level
        CHECK(!estep(f, 0).coarse_issued && estep(f, 0).main.kind == KERNEL_TILED);
        f.coarse_pass = 2;
        CHECK(estep(f, 0).coarse_issued);
    }
    {  // "lean memory": the build releases the stream and call_rows; the fine level is fine8 from this E-step on, with its allowance
        Facts f = flagship();
        f.lean_memory = true;
        const Ran r = estep(f, 0);
        CHECK(r.built && r.released && r.main.kind == KERNEL_FINE8 && r.main.cpg == 2 && !r.after.tile_stream && !r.after.call_rows);
        CHECK(fine_allowance(f, WALK_TILE_STREAM) == GUARD_PER_CALL_PLAIN && fine_allowance(f, WALK_COARSE_RECORDS) == guard_per_call_fine8(2));
        Facts g = r.after;
        g.logits_kept = g.dict_candidate = true;  // the prior table again, logits kept: no dictionary without call_rows
        CHECK(!dictionary_admissible(g) && estep(g, 3).main.kind == KERNEL_FINE8);
        g.mode = MODE_EXACT;
        CHECK(estep(g, 3).main.kind == KERNEL_DIRECT && estep(g, 3).walk == WALK_BARCODE_MAJOR);
    }
    {  // "clip below binary16's normal range" / "small singlet tables": no coarse pass
        Facts f = flagship();
        f.lo = 1e-5f;
        CHECK(!coarse_capable(f, f.lo) && !estep(f, 0).coarse_issued && estep(f, 0).main.kind == KERNEL_TILED);
        f = flagship(), f.G = f.K = 16;
        CHECK(!coarse_capable(f, f.lo) && estep(f, 0).main.kind == KERNEL_DIRECT && estep(f, 0).main.L == 16);
        f.G = f.K = 17;
        CHECK(estep(f, 0).main.kind == KERNEL_TILED_TWO_CALLS && estep(f, 0).coarse.cpg == 4);
        f.G = f.K = 128;
        CHECK(estep(f, 0).main.kind == KERNEL_TILED && estep(f, 0).main.A == 2 && estep(f, 0).coarse.cpg == 1);
        f.G = f.K = 129;
        CHECK(estep(f, 0).main.kind == KERNEL_DIRECT && estep(f, 0).main.A == 4 && !estep(f, 0).coarse_issued);
    }
    {  // "exact mode": one barcode per wavefront unless the schedule is forced, and then only from 33 genotypes
        Facts f = flagship();
        f.mode = MODE_EXACT;
        CHECK(estep(f, 0).branch == BR_PLAIN && estep(f, 0).main.kind == KERNEL_DIRECT && !estep(f, 0).main.fast);
        f.schedule = 2;
        CHECK(estep(f, 0).main.kind == KERNEL_TILED && !estep(f, 0).main.fast);
        f.G = f.K = 32;
        CHECK(estep(f, 0).main.kind == KERNEL_DIRECT);
    }
    {  // "narrow doublet tables": packed (G = 8, K = 36: 8 lanes x 5 slots), exact also in the guarded mode; long rows beyond an eighth: not
        Facts f = doublets_of(8, 200000);
        int lanes = 0, slots = 0;
        CHECK(estep_packed_shape(36, 8, &lanes, &slots) && lanes == 8 && slots == 5);
        CHECK(estep(f, 9).branch == BR_PACKED && !estep(f, 9).fast && packed_candidate(f).n_long == 2000);
        f.n_long_rows[0] = 25001;
        CHECK(estep(f, 9).branch == BR_GUARDED && estep(f, 9).main.kind == KERNEL_DIRECT && estep(f, 9).main.L == 64 && estep(f, 9).main.fast);
        f.packing = 3;
        CHECK(estep(f, 9).branch == BR_PACKED);
        f.packing = 2;
        CHECK(estep(f, 9).branch == BR_PACKED && packed_candidate(f).n_long == 0);
        f.packing = 1, f.row_statistic = false;
        CHECK(estep(f, 9).branch == BR_GUARDED);
        f = doublets_of(8, 200000), f.mode = MODE_FAST;
        CHECK(estep(f, 9).branch == BR_PLAIN && estep(f, 9).main.fast);
    }
    {  // "doublet tables of 257 .. 512 options": lane per option in the exact mode, workgroup per barcode with the tolerance arithmetic
        Facts f = doublets_of(31, 20000);  // K = 496
        f.segments = true;
        CHECK(estep(f, 9).branch == BR_GUARDED && estep(f, 9).main.kind == KERNEL_PAIR_BLOCKS && estep(f, 9).main.threads == 256 &&
              estep(f, 9).redo.kind == KERNEL_DIRECT && estep(f, 9).redo.A == 8);
        f.with_prior = true;  // the guard of the workgroup-per-barcode forms does not cover prior logits: exact
        CHECK(!guarded(f) && estep(f, 9).branch == BR_PLAIN && estep(f, 9).main.kind == KERNEL_DIRECT && !estep(f, 9).main.fast);
        f = doublets_of(22, 20000), f.segments = true;  // K = 253: split rows on 64 lanes
        CHECK(estep(f, 9).main.kind == KERNEL_DIRECT_SPLIT && estep(f, 9).main.A == 4 && estep(f, 9).redo.kind == KERNEL_DIRECT);
    }
    {  // "wide doublet tables": K = 8256: the dictionary's block form where the table allows it; else pair blocks of 512 threads, the redo in tiles of 17
        Facts f = doublets_of(128, 130000);
        f.dict_candidate = f.logits_kept = true;
        CHECK(estep(f, 3).branch == BR_DICT_BLOCK && estep(f, 5).branch == BR_GUARDED);
        const Ran r = estep(f, 5);
        CHECK(r.main.kind == KERNEL_PAIR_BLOCKS && r.main.threads == 512 && r.main.launches == 3 && f.n_pair_blocks == 1429);
        CHECK(r.redo.kind == KERNEL_BLOCK_TILES && r.redo.tile == 17 && r.redo.launches == 2);
        f.mode = MODE_FAST, f.n_pair_blocks = 0;
        CHECK(estep(f, 5).main.kind == KERNEL_BLOCK_TILES && estep(f, 5).main.tile == 6 && estep(f, 5).main.launches == 6);
        f = doublets_of(128, 130000), f.lean_memory = true;  // a run with doublets never reads the tile-major stream
        CHECK(unused_stream_release_due(f) && !estep(f, 5).after.tile_stream);
    }
    {  // "singlets beyond 1024 genotypes": refused
        Facts f = flagship();
        f.G = f.K = 1025;
        CHECK(estep(f, 0).main.kind == KERNEL_REFUSED);
        f.G = f.K = 1024;
        CHECK(estep(f, 0).main.kind == KERNEL_DIRECT && estep(f, 0).main.A == 16 && estep(f, 0).main.U == 2);
    }
    {  // "sliced with lists of changed rows": the conversion leaves the binary16 table valid
        Facts f = flagship();
        f.sliced = f.table_lists = true;
        CHECK(estep(f, 0).converted && estep(f, 0).after.prob16_valid);
        f.table_lists = false;
        CHECK(estep(f, 0).converted && !estep(f, 0).after.prob16_valid);
    }
}

}  // namespace

int main()
{
    const long long n = walk_all();
    table_rows();
    std::printf("estep plan: %lld combinations walked, %lld failures\n", n, failures);
    return failures ? 1 : 0;
}
