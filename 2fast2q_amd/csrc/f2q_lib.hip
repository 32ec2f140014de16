// f2q_lib.hip -- libf2q_hip.so: the one translation unit.  Kernels live in f2q_count_kernels.h and
// f2q_aux_kernels.h, the per-lane logic in f2q_device.h; this file holds the host side and the C ABI of include/f2q.h.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <unordered_map>
#include <mutex>
#include <thread>
#include <vector>

#include "f2q_device.h"
#include "f2q_host.h"
#include "f2q_synth.h"
#include "f2q_reader.h"

using namespace f2q;

#include "f2q_count_kernels.h"
#include "f2q_part_kernels.h"
#include "f2q_aux_kernels.h"
#include "f2q_pair_kernels.h"
#include "f2q_inflate_kernels.h"
#include "f2q_assign_kernels.h"
#include "f2q_ec_collapse_kernels.h"
#include "f2q_umi_kernels.h"
#include "f2q_demux_kernels.h"
#include "f2q_strand_kernels.h"
#include "f2q_stagger_kernels.h"
#include "f2q_indel_kernels.h"
#include "f2q_parts_kernels.h"

// ===============================================================================================
// host side
// ===============================================================================================
struct f2q_block {
    PackedBlock pb{};
    RawBlock rb{};
    std::vector<void *> allocs;
    uint64_t n_reads = 0, n_general = 0, dev_bytes = 0;
    uint64_t raw_key_bytes = 0;            // upper bound of the key bytes the raw records can produce (Extract+Count arena sizing)
};

// The raw-record modes of a Counter context.  They exclude each other: f2q_ctx::raw_mode names the one in place, and what
// is said when a call meets it is built from its row of RAW_MODES (raw_mode_enter and the raw_mode_* refusals below).
enum RawMode { RAW_NONE, RAW_UMI, RAW_DEMUX, RAW_STRAND, RAW_STAGGER, RAW_INDEL, RAW_PARTS };
struct RawModeRow {
    const char *phrase;      // the context in messages
    const char *setter;      // the call that made it one
    const char *what;        // what the mode adds, in "X and Y are not combined"
    bool pairs_ok;           // merged pairs are counted too (else single reads, single raw records only)
    bool once;               // the setter comes once (else it may be called again, and with 0 to take the mode back)
    const char *mate2;       // what f2q_set_mate2 says of such a context
    const char *unmerged;    // what several ranks cannot merge
};
static const RawModeRow RAW_MODES[] = {
    {"a plain context", "", "", true, false, "", ""},
    {"a UMI context (f2q_set_umi / f2q_set_umi_header / f2q_set_umi_paired)", "f2q_set_umi", "UMIs", true, true,
     "counts single reads only: f2q_set_mate2 comes first, then f2q_set_umi_paired", "the sets"},
    {"a demultiplexing context (f2q_set_sample_barcodes)", "f2q_set_sample_barcodes", "sample barcodes", false, true, "counts single reads only", "the matrices"},
    {"a context with a strand mode (f2q_set_strand: rev / both)", "f2q_set_strand", "a strand mode", false, true, "counts single reads only", "the reverse-strand counts"},
    {"a stagger context (f2q_set_stagger)", "f2q_set_stagger", "a stagger", false, false, "counts single reads only", "the offset histograms"},
    {"an indel context (f2q_set_indel)", "f2q_set_indel", "indel reads", false, false, "counts single reads only", "the indel counts"},
    {"a parts context (f2q_set_parts)", "f2q_set_parts", "part verdicts", true, true,
     "keeps its windows: f2q_set_mate2 comes first, then f2q_set_parts", "the tables and sets"},
};

// A set of pairs in device memory that grows with what is counted: (feature, UMI) of a UMI context, (part 1, part 2) of
// the recombinants of a parts context.  *dev is the kernels' view of it, inside the owner's device struct.
struct PairSet {
    UmiDev *dev;
    const char *name;                    // "<name> set" in messages and traces
    bool keep_reads;                     // dev->reads[] lives and dies with dev->slots[]
    std::vector<void *> set_allocs;      // slots[] (and reads[])
    uint64_t n_slots = 0, min_slots = (uint64_t)1 << 16;     // F2Q_UMI_SLOTS / F2Q_PARTS_SLOTS: the first set's size (tests: growth from a small one)
    uint64_t held_ub = 0;                // pairs held, an upper bound: every record launched since the last exact reading taken as new
    uint64_t rehashes = 0;
};

struct f2q_ctx {
    f2q_params prm{};
    std::vector<std::string> up_s, down_s;
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_a = nullptr, ev_b = nullptr, ev_k0 = nullptr, ev_k1 = nullptr;
    std::vector<hipEvent_t> q_ev;          // f2q_count_resident_queued: a pair of events per queued step
    uint32_t q_n = 0;                      // steps queued since the last f2q_queued_times
    hipStream_t copy_stream = nullptr;   // PieceStream: the text of the next piece travels while this one is counted
    hipEvent_t ev_copy = nullptr;
    RunDev run_h{};
    RunDev *run_d = nullptr;
    PackPlan plan{};
    int n_mate1 = 0;                     // f2q_set_mate2: a paired context, windows [0, n_mate1) of the run lie in mate 1
    bool rc2 = false;                    // ... and mate 2 is taken reverse-complemented
    // library
    bool have_lib = false;
    HostIndex ix;
    LibDev lib_h{};
    LibDev *lib_d = nullptr;
    std::vector<void *> lib_allocs;
    uint64_t *guide_keys_d = nullptr;
    std::vector<uint64_t> synth_keys;    // generator guides set by f2q_synth_guides (else the library's)
    uint64_t *synth_keys_d = nullptr;
    uint32_t synth_glen = 0;
    // accumulators: counts[n_features] then stats[5]
    unsigned long long *acc_d = nullptr;
    uint64_t acc_n = 0;
    // f2q_reset_counts leaves the clear of acc_d pending: the step's first k_reduce_slabs stores instead of adding
    // (reduce_slabs), whatever else reads or writes acc_d first clears it (acc_ready).  acc_eager: the raw pointer is out
    // (f2q_counts_device_ptr), whoever holds it may read at any time, so a reset clears at once
    bool acc_pending = false, acc_eager = false;
    unsigned long long *carry_d = nullptr;   // Accum::carry, max(n_features, 1) words, zero between launches
    uint32_t *slab_d = nullptr;          // per-workgroup histogram rows of the v2 kernel
    size_t slab_n = 0;
    unsigned long long *stat_slab_d = nullptr;   // per-workgroup stats rows of 8
    size_t stat_slab_n = 0;
    uint32_t *hit_buf_d = nullptr;       // large libraries: feature index per read slot of the block being counted
    size_t hit_buf_n = 0;
    // Extract+Count table
    EcDev ec{};
    std::vector<void *> ec_allocs;       // byte-string side: slots, entry arrays, arena
    std::vector<void *> ec_allocs64;     // single-word side: k64_*
    std::vector<void *> ec_allocs_ctr;   // the four counters (outlive the growth of either side)
    // raw records of an Extract+Count block are decided on a second stream while the packed tiles are counted
    hipStream_t aux_stream = nullptr;
    hipEvent_t ev_aux0 = nullptr, ev_aux1 = nullptr;
    bool aux_busy = false;
    uint64_t ec_slots = 0;
    // hot keys of the single-word table (EcHot): learnt from the first hot_learn reads of a sample, kept in LDS by
    // k_extract_anchor_hot; `defer` lists the reads that kernel sets aside for k_ec_deferred
    EcHot hot{};
    std::vector<void *> hot_allocs;
    bool hot_valid = false, no_hot = false;
    uint64_t hot_learn = (uint64_t)1 << 18, ec_learned = 0;
    unsigned long long *defer_d = nullptr; size_t defer_cap = 0;
    uint64_t reads_seen = 0;             // global read index of the next block's read 0
    // Extract+Count with a library (f2q_set_assign_library / f2q_ec_assign): an index of its own -- the context's lib_d
    // stays the empty library the counting kernels are handed -- a result vector of its own (counts then 5 stats then
    // the bad-entry word) and the per-key arrays of the last assign, valid while asg_gen == ec_gen
    bool have_asg = false;
    HostIndex asg_ix;
    LibDev asg_lib_h{};
    LibDev *asg_lib_d = nullptr;
    std::vector<void *> asg_lib_allocs, asg_allocs;
    unsigned long long *asg_acc_d = nullptr;
    AssignDev asg{};
    uint64_t asg_nb = 0, asg_nw = 0;     // entries / slots the per-key arrays cover
    uint64_t ec_gen = 1, asg_gen = 0;    // ec_gen: bumped by every count call, reset and table growth
    // extracted keys one base apart collapsed (f2q_ec_collapse): root[] and cluster[] of the last call over the single-word
    // slots (null: every key is its own centroid), valid while ecc_gen == ec_gen
    std::vector<void *> ecc_allocs;
    uint32_t *ecc_root = nullptr;
    unsigned long long *ecc_cluster = nullptr;
    uint64_t ecc_nb = 0, ecc_nw = 0, ecc_gen = 0;    // entries / slots the per-key arrays cover
    // The raw-record modes (RAW_MODES): at most one is in place.  Each sends every read down the raw-record road
    // (raw_road_enter) to a kernel of its own; its parameters and device memory live in its struct below
    RawMode raw_mode = RAW_NONE;
    bool env_general = false;            // what F2Q_FORCE_GENERAL said before the context was sent down the raw-record road
    // distinct UMIs per feature (f2q_set_umi): the set of (feature, UMI) pairs, umis[n_features] and the counters.  The set
    // outlives the pieces of a file; pairset_reserve sizes it before every launch
    struct {
        UmiDev dev{};
        PairSet set{&dev, "UMI", false};     // keep_reads: f2q_set_umi_reads
        std::vector<void *> fix_allocs;  // umis[] and the counters
        bool pair_stage = false;         // f2q_set_umi_paired: k_count_umi_pair<.., true> (F2Q_UMI_PAIR_STAGE)
        int32_t hdr_sep = 0;             // f2q_set_umi_header: the separator byte (0: the UMI is not in the header); the length is dev.length
    } umi;
    // inline sample barcodes (f2q_set_sample_barcodes): the barcode table, the count matrix [(n + 1)][n_features], the five
    // reference counters per sample and the five verdict counters; they live across pieces and counting calls
    struct {
        DemuxDev dev{};
        DemuxTable tab;                  // the host's copy of the table (uploaded once, with the first allocation)
        std::vector<void *> allocs;      // table, matrix, sstats + verdicts
        uint64_t matrix_n = 0;           // words of dev.matrix
        bool lds_table = false;          // k_count_demux<true> (F2Q_DEMUX_TABLE=lds, and the table fits)
    } demux;
    // read orientation (f2q_set_strand): reads assigned on the reverse strand per feature and the four strand counters; they
    // live across pieces and counting calls
    struct {
        int32_t mode = 0;                // F2Q_STRAND_REV / _BOTH of a RAW_STRAND context
        StrandDev dev{};
        std::vector<void *> allocs;      // rev_counts + extra, one allocation
        uint64_t words = 0;              // of that allocation: max(n_features, 1) + 4
    } strand;
    // staggered libraries (f2q_set_stagger): the window tried at the starts s .. s + n, the reads assigned at each offset
    struct {
        int32_t n = 0;                   // 1 .. 32 on a RAW_STAGGER context
        StaggerDev dev{};
        std::vector<void *> allocs;      // the two histograms, one allocation of 2 * (n + 1) words
    } stagger;
    // one-base insertions and deletions (f2q_set_indel): the deletion-variant table, the per-feature counts, the two position
    // histograms and the four totals; built once the flag and a library are both known (indel_install)
    struct {
        IndelDev dev{};
        std::vector<void *> allocs;      // the table's two arrays; the counters, one allocation of `words` words
        uint64_t words = 0;              // 2 * max(n_features, 1) + 2 * L + 4
    } indel;
    // pair libraries with each part matched alone (f2q_set_parts): the two part libraries (indices of their own, as the
    // assign library has one), the pair table, parts_counts / the marginals / the six class counters (one allocation) and
    // the recombinant set, which outlives the pieces of a file; pairset_reserve sizes it before every launch
    struct {
        PartsDev dev{};
        PairSet set{&dev.rec, "recombinant", true};
        PartsTable tab;                  // the host's copy: part texts, feature -> ids, the pair table
        HostIndex ix[2];
        LibDev lib_h[2]{};
        std::vector<void *> lib_allocs[2], fix_allocs;   // the part libraries / tables and counters
        uint64_t words = 0;              // of the counters' allocation: nf + n1 + n2 + 6 (each count at least 1)
    } parts;
    bool counted = false;                // a counting launch has been made (f2q_set_umi comes before the first)
    uint32_t last_path = 0;              // F2Q_PATH_* of the last packed-tile launch (f2q_timing.path)
    int n_cu = 256;
    bool force_generic = false;           // F2Q_GENERIC=1: run-time window geometry even where a specialisation exists
    bool host_pack = false;               // F2Q_HOST_PACK=1: frame/classify/pack on the host (the round-1 first path; A/B runs)
    bool force_general = false;           // F2Q_FORCE_GENERAL=1: every read through the byte-exact general kernel (cross-checks)
    bool force_v1 = false;                // F2Q_FORCE_V1=1: keep the one-read-per-lane kernel (A/B runs)
    bool no_lt = false;                   // F2Q_NO_LT=1: never the LDS-table kernel (A/B runs, cross-checks)
    uint32_t lt_max_wgs = 0;              // F2Q_LT_WGS=n: at most n workgroups of the kernels that count in u16 LDS counters -- k_count_fixed4_lds, k_count_anchor_lt, k_count_anchor_pairs (tests: many reads per histogram) -- and of k_part_scatter, k_count_fixed4, k_count_multi4, k_extract_anchor_hot, k_extract_fixed4_hot (tests: several tiles per wave on a small block)
    bool no_pt = false;                   // F2Q_NO_PT=1: never the partitioned-table kernels (A/B runs, cross-checks)
    uint64_t pt_chunk_reads = (uint64_t)1 << 28;   // F2Q_PT_CHUNK: most reads per scatter/count round of the partitioned path (1.7 GB of streams per 200 M reads; 400 M reads in two rounds run 8 % faster than in six)
    uint64_t pt_min_reads = (uint64_t)1 << 21;     // F2Q_PT_MIN_READS: smaller blocks keep the packed-table kernel (three launches and the
                                                   // tables' way into LDS do not pay for a block that small)
    // scratch of the partitioned path (k_part_*): entry streams and their lengths, the two slabs, the stats rows
    PartScratch pt_s{};
    size_t pt_streams_n = 0, pt_cnt_n = 0, pt_slab0_n = 0, pt_slab1_n = 0;
    uint32_t *pt_slab0_d = nullptr, *pt_slab1_d = nullptr;
    unsigned long long *pt_stat_d = nullptr; size_t pt_stat_n = 0;
    // device memory freed by blocks / scratch is kept (idle, after a stream sync) for the next piece of the same
    // size class: a streamed file costs ~20 allocations per piece otherwise
    std::multimap<size_t, void *> dev_idle;
    std::unordered_map<void *, size_t> dev_size;
    size_t dev_idle_bytes = 0, dev_idle_cap = (size_t)8 << 30;
    std::string err;
    // F2Q_TRACE=1: wall-clock split of the host entry points, printed by f2q_count_file (diagnostics only)
    bool trace = false, trace_sync = false;
    double tr_frame = 0, tr_count = 0, tr_free = 0, tr_copy = 0, tr_malloc = 0, tr_hipfree = 0, tr_reserve = 0;
    uint64_t n_malloc = 0, n_hipfree = 0, n_reuse = 0, n_rehash = 0;
};

static thread_local std::string g_create_err;
static inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static int fail(f2q_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg; else g_create_err = msg;
    return code;
}

#define HIPC(ctx, call)                                                                             \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return fail(ctx, F2Q_EHIP, std::string(#call) + ": " + hipGetErrorString(e_));          \
    } while (0)

static int dev_get(f2q_ctx *c, size_t bytes, void **out)
{
    bytes = (bytes + 255) & ~(size_t)255;
    auto it = c->dev_idle.lower_bound(bytes);
    if (it != c->dev_idle.end() && it->first <= bytes + bytes / 4 + (64 << 10)) {
        *out = it->second; c->dev_idle_bytes -= it->first; c->dev_idle.erase(it);
        c->n_reuse++;
        return F2Q_OK;
    }
    void *p = nullptr;
    const double m0 = now_ms();
    hipError_t e = hipMalloc(&p, bytes);
    c->tr_malloc += now_ms() - m0; c->n_malloc++;
    if (e != hipSuccess && !c->dev_idle.empty()) {           // give the idle memory back and retry once
        for (auto &kv : c->dev_idle) { c->dev_size.erase(kv.second); (void)hipFree(kv.second); }
        c->dev_idle.clear(); c->dev_idle_bytes = 0;
        e = hipMalloc(&p, bytes);
    }
    if (e != hipSuccess) return fail(c, F2Q_EHIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    c->dev_size[p] = bytes;
    *out = p;
    return F2Q_OK;
}
template <class T>
static int dev_upload(f2q_ctx *c, const T *src, size_t n, T **dst, std::vector<void *> &owner)
{
    void *p = nullptr;
    int rc = dev_get(c, (n ? n : 1) * sizeof(T), &p);
    if (rc) return rc;
    owner.push_back(p);
    if (n) HIPC(c, hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    *dst = (T *)p;
    return F2Q_OK;
}
template <class T>
static int dev_alloc(f2q_ctx *c, size_t n, T **dst, std::vector<void *> &owner, int fill = -1)
{
    void *p = nullptr;
    size_t bytes = (n ? n : 1) * sizeof(T);
    int rc = dev_get(c, bytes, &p);
    if (rc) return rc;
    owner.push_back(p);
    if (fill >= 0) HIPC(c, hipMemsetAsync(p, fill, bytes, c->stream));
    *dst = (T *)p;
    return F2Q_OK;
}
// memory goes back to the idle list only once nothing queued on the stream can still touch it
static void free_all(f2q_ctx *c, std::vector<void *> &v)
{
    if (v.empty()) return;
    if (!c) { for (void *p : v) (void)hipFree(p); v.clear(); return; }      // block outliving its context
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (void *p : v) {
        auto it = c->dev_size.find(p);
        if (it != c->dev_size.end() && c->dev_idle_bytes + it->second <= c->dev_idle_cap) {
            c->dev_idle.emplace(it->second, p); c->dev_idle_bytes += it->second;
        } else {
            if (it != c->dev_size.end()) c->dev_size.erase(it);
            const double f0 = now_ms();
            (void)hipFree(p);
            c->tr_hipfree += now_ms() - f0; c->n_hipfree++;
        }
    }
    v.clear();
}
// device allocations that go back when the scope ends, on every return path: free_all waits for the stream first
struct DevScope {
    f2q_ctx *const c; std::vector<void *> v;
    explicit DevScope(f2q_ctx *ctx, void *p = nullptr) : c(ctx) { if (p) v.push_back(p); }
    ~DevScope() { free_all(c, v); }
    DevScope(const DevScope &) = delete;
};
static int hip_rc(f2q_ctx *c, hipError_t e) { return e == hipSuccess ? F2Q_OK : fail(c, F2Q_EHIP, hipGetErrorString(e)); }
// the calls for single reads refuse a paired context, and the other way round
static int single_only(f2q_ctx *c) { return c->n_mate1 ? fail(c, F2Q_ESTATE, "a paired context (f2q_set_mate2) counts pairs only: use the f2q_*_paired calls") : F2Q_OK; }
static int paired_only(f2q_ctx *c) { return c->n_mate1 ? F2Q_OK : fail(c, F2Q_ESTATE, "not a paired context: call f2q_set_mate2 first"); }

// ---- the raw-record modes: one refusal path -----------------------------------------------------------------------------
// What every setter of a mode asks before it changes anything (`who`: the setter as it is named in messages).  All of these
// are F2Q_ESTATE; where several apply the first of this order speaks: a Counter context; single reads (a mode that takes no
// merged pairs); the setter's own shape requirement (`shape`: its complaint about windows or reads, empty when there is none); no other mode
// in place; the mode not in place already (once); nothing counted yet.  f2q_set_stagger and f2q_set_indel, which can be
// called again and with 0, ask the last question themselves, first of all.
static int raw_mode_enter(f2q_ctx *c, RawMode mode, const char *who, const std::string &shape = std::string())
{
    const RawModeRow &in_place = RAW_MODES[c->raw_mode], &mine = RAW_MODES[mode];
    if (c->prm.mode != 0) return fail(c, F2Q_ESTATE, std::string(who) + " takes a Counter context, not Extract+Count");
    if (!mine.pairs_ok && c->n_mate1) return fail(c, F2Q_ESTATE, std::string(who) + " takes single reads, not a paired context (f2q_set_mate2)");
    if (!shape.empty()) return fail(c, F2Q_ESTATE, std::string(who) + " " + shape);
    if (c->raw_mode != RAW_NONE && c->raw_mode != mode)
        return fail(c, F2Q_ESTATE, std::string(who) + " on " + in_place.phrase + ": " + mine.what + " and " + in_place.what + " are not combined");
    if (mine.once && c->raw_mode == mode) return fail(c, F2Q_ESTATE, std::string(who) + " comes once: this is " + in_place.phrase + " already");
    if (c->counted) return fail(c, F2Q_ESTATE, std::string(who) + " comes before counting");
    return F2Q_OK;
}
// f2q_set_mate2 on a context with a mode in place
static int raw_mode_no_mate2(f2q_ctx *c)
{
    if (c->raw_mode == RAW_NONE) return F2Q_OK;
    return fail(c, F2Q_ESTATE, std::string(RAW_MODES[c->raw_mode].phrase) + " " + RAW_MODES[c->raw_mode].mate2);
}
// a share of a file (rank of world > 1) on a context with a mode in place: what the mode gathers is not merged
static int raw_mode_one_rank(f2q_ctx *c, uint32_t world)
{
    if (c->raw_mode == RAW_NONE || world <= 1) return F2Q_OK;
    return fail(c, F2Q_ESTATE, std::string(RAW_MODES[c->raw_mode].phrase) + " counts whole files: " + RAW_MODES[c->raw_mode].unmerged + " of several ranks are not merged");
}
// a block on a context with a mode in place (launch_block): packed tiles, or records of the wrong kind, say that the block
// was made before the mode was set
static int raw_mode_block(f2q_ctx *c, const f2q_block *b)
{
    const RawModeRow &row = RAW_MODES[c->raw_mode];
    bool stale = b->pb.n_tiles != 0;
    if (!row.pairs_ok) stale = stale || b->rb.len1;
    else if (c->raw_mode == RAW_PARTS) stale = stale || (b->rb.n && (b->rb.len1 != nullptr) != (c->n_mate1 != 0));
    if (stale) return fail(c, F2Q_ESTATE, std::string("the block was packed before ") + row.setter + ": " + row.phrase + " counts " + (row.pairs_ok ? "" : "single ") + "raw records only");
    if (c->raw_mode == RAW_UMI && c->umi.hdr_sep && b->rb.n && !b->rb.hdr_umi)
        return fail(c, F2Q_ESTATE, "the block was made before f2q_set_umi_header (or without headers): its records carry no header UMI");
    return F2Q_OK;
}
// Every read takes the raw-record road, as F2Q_FORCE_GENERAL=1 sends it, to the kernel of `mode` (launch_raw);
// f2q_set_features keeps it that way.  Last in a setter: whatever can fail has been done.
static void raw_road_enter(f2q_ctx *c, RawMode mode)
{
    if (c->raw_mode == RAW_NONE) c->env_general = c->force_general;
    c->raw_mode = mode;
    c->force_general = true;
    c->plan.fast_fixed = false; c->plan.fast_anchor = false; c->plan.multi = false; c->plan.multi_pair = false;
    c->plan.inband_n = false; c->plan.n_only = false;
}
// the first size of a pair set: F2Q_UMI_SLOTS / F2Q_PARTS_SLOTS rounded up to a power of two
static uint64_t pairset_min_slots_from_env(const char *name)
{
    uint64_t slots = (uint64_t)1 << 16;
    const char *e = getenv(name);
    if (e && atol(e) > 0) { slots = 2; while (slots < (uint64_t)atol(e) && slots < (1ull << 32)) slots <<= 1; }
    return slots;
}
// bytes of text per piece of a streamed file; F2Q_FILE_CHUNK overrides (tests)
static size_t file_chunk_bytes(size_t dflt) { const char *e = getenv("F2Q_FILE_CHUNK"); return e && atol(e) >= 4096 ? (size_t)atol(e) : dflt; }

extern "C" int f2q_version(void) { return F2Q_ABI_VERSION; }

#ifndef F2Q_BUILD_ID
#define F2Q_BUILD_ID "unknown"
#endif
// the "F2Q_BUILD_ID=" prefix lets build() find the id in the file without loading it
static const char g_build_id[] = "F2Q_BUILD_ID=" F2Q_BUILD_ID;
extern "C" const char *f2q_build_id(void) { return g_build_id + 13; }

extern "C" const char *f2q_last_error(const f2q_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

extern "C" void *f2q_stream(f2q_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

static int setup_run(f2q_ctx *c)
{
    f2q_params p = c->prm;
    for (int i = 0; i < p.n_upstream && i < F2Q_MAX_ITER; i++) p.upstream[i] = c->up_s[i].c_str();
    for (int i = 0; i < p.n_downstream && i < F2Q_MAX_ITER; i++) p.downstream[i] = c->down_s[i].c_str();
    std::string err;
    int rc = fill_run(p, c->run_h, err, c->n_mate1);
    if (rc) return fail(c, rc, err);
    c->plan = make_plan(c->run_h);
    c->plan.rc2 = c->rc2;
    if (c->force_general) { c->plan.fast_fixed = false; c->plan.fast_anchor = false; c->plan.multi_pair = false; }
    return F2Q_OK;
}

// the index ix on the device: L = its host-side descriptor, *lib_d = the device copy of L, owner = the allocations
static int upload_index(f2q_ctx *c, const HostIndex &ix, LibDev &L, LibDev **lib_d, std::vector<void *> &owner, uint64_t **guide_keys)
{
    free_all(c, owner);
    memset(&L, 0, sizeof L);
    L.n_features = ix.n_features;
    L.n_irregular = ix.n_irregular;
    memcpy(L.grp, ix.grp, sizeof L.grp);
    L.pk = ix.pk;
    memcpy(L.mpk, ix.mpk, sizeof L.mpk);
    L.mw_ok = ix.mw_ok;
    uint64_t *tk; uint32_t *ti; uint8_t *fb; uint32_t *fo; uint32_t *ir; uint64_t *gk; uint64_t *pt;
    int rc;
    if ((rc = dev_upload(c, ix.tab_keys.data(), ix.tab_keys.size(), &tk, owner))) return rc;
    if ((rc = dev_upload(c, ix.tab_idx.data(), ix.tab_idx.size(), &ti, owner))) return rc;
    if ((rc = dev_upload(c, ix.feat_bytes.data(), ix.feat_bytes.size(), &fb, owner))) return rc;
    if ((rc = dev_upload(c, ix.feat_off.data(), ix.feat_off.size(), &fo, owner))) return rc;
    if ((rc = dev_upload(c, ix.irr_ids.data(), ix.irr_ids.size(), &ir, owner))) return rc;
    if ((rc = dev_upload(c, ix.key2.data(), ix.key2.size(), &gk, owner))) return rc;
    if ((rc = dev_upload(c, ix.ptab.data(), ix.ptab.size(), &pt, owner))) return rc;
    L.ptab = pt;
    {
        uint32_t *lt_tags, *lt_feat; uint16_t *lt_slot;
        if ((rc = dev_upload(c, ix.lt_tags.data(), ix.lt_tags.size(), &lt_tags, owner))) return rc;
        if ((rc = dev_upload(c, ix.lt_feat_of.data(), ix.lt_feat_of.size(), &lt_feat, owner))) return rc;
        if ((rc = dev_upload(c, ix.lt_slot_of.data(), ix.lt_slot_of.size(), &lt_slot, owner))) return rc;
        L.lt = ix.lt; L.lt.tags = lt_tags; L.lt.feat_of = lt_feat; L.lt.slot_of = lt_slot;
        uint64_t *pw_tab;
        if ((rc = dev_upload(c, ix.pw_tab.data(), ix.pw_tab.size(), &pw_tab, owner))) return rc;
        L.pw = ix.pw; L.pw.tab = pw_tab;
        { const char *e = getenv("F2Q_NO_PW"); if (e && e[0] == '1') L.pw.ok = 0; }      // A/B runs: the joined key as a string (byte-string index)
        uint32_t *pt_t0, *pt_t1, *pt_ps, *pt_s1, *pt_fo, *pt_f0; uint16_t *pt_s0;
        if ((rc = dev_upload(c, ix.pt_tags0.data(), ix.pt_tags0.size(), &pt_t0, owner))) return rc;
        if ((rc = dev_upload(c, ix.pt_tags1.data(), ix.pt_tags1.size(), &pt_t1, owner))) return rc;
        if ((rc = dev_upload(c, ix.pt_pstart.data(), ix.pt_pstart.size(), &pt_ps, owner))) return rc;
        if ((rc = dev_upload(c, ix.pt_slot0_of.data(), ix.pt_slot0_of.size(), &pt_s0, owner))) return rc;
        if ((rc = dev_upload(c, ix.pt_slot1_of.data(), ix.pt_slot1_of.size(), &pt_s1, owner))) return rc;
        if ((rc = dev_upload(c, ix.pt_feat_of.data(), ix.pt_feat_of.size(), &pt_fo, owner))) return rc;
        if ((rc = dev_upload(c, ix.pt_feat0_of.data(), ix.pt_feat0_of.size(), &pt_f0, owner))) return rc;
        L.pt = ix.pt; L.pt.tags0 = pt_t0; L.pt.tags1 = pt_t1; L.pt.pstart = pt_ps; L.pt.slot0_of = pt_s0; L.pt.slot1_of = pt_s1;
        L.pt.feat_of = pt_fo; L.pt.feat0_of = pt_f0;
        GkGroup *gk_grp; uint32_t *gk_tab, *gk_ids;
        if ((rc = dev_upload(c, ix.gk_groups.data(), ix.gk_groups.size(), &gk_grp, owner))) return rc;
        if ((rc = dev_upload(c, ix.gk_tab.data(), ix.gk_tab.size(), &gk_tab, owner))) return rc;
        if ((rc = dev_upload(c, ix.gk_ids.data(), ix.gk_ids.size(), &gk_ids, owner))) return rc;
        L.gk.n_groups = ix.n_features ? (uint32_t)ix.gk_groups.size() : 0u; L.gk.grp = gk_grp; L.gk.tab = gk_tab; L.gk.ids = gk_ids;
        unsigned long long *gk_fw; uint32_t *gk_fwoff;
        if ((rc = dev_upload(c, ix.gk_fw.data(), ix.gk_fw.size(), &gk_fw, owner))) return rc;
        if ((rc = dev_upload(c, ix.gk_fwoff.data(), ix.gk_fwoff.size(), &gk_fwoff, owner))) return rc;
        L.gk.fw = gk_fw; L.gk.fwoff = gk_fwoff;
    }
    L.tab_keys = tk; L.tab_idx = ti; L.feat_bytes = fb; L.feat_off = fo; L.irr_ids = ir;
    if (guide_keys) *guide_keys = gk;
    LibDev *ld;
    if ((rc = dev_upload(c, &L, 1, &ld, owner))) return rc;
    *lib_d = ld;
    HIPC(c, hipStreamSynchronize(c->stream));
    return F2Q_OK;
}
static int upload_lib(f2q_ctx *c) { return upload_index(c, c->ix, c->lib_h, &c->lib_d, c->lib_allocs, &c->guide_keys_d); }

static int alloc_acc(f2q_ctx *c, uint64_t n_features)
{
    if (c->acc_d) { (void)hipFree(c->acc_d); c->acc_d = nullptr; }
    if (c->carry_d) { (void)hipFree(c->carry_d); c->carry_d = nullptr; }
    c->acc_n = n_features + 5;
    const size_t carry_n = (size_t)std::max<uint64_t>(n_features, 1);
    HIPC(c, hipMalloc((void **)&c->acc_d, c->acc_n * sizeof(unsigned long long)));
    HIPC(c, hipMalloc((void **)&c->carry_d, carry_n * sizeof(unsigned long long)));
    HIPC(c, hipMemsetAsync(c->acc_d, 0, c->acc_n * sizeof(unsigned long long), c->stream));
    HIPC(c, hipMemsetAsync(c->carry_d, 0, carry_n * sizeof(unsigned long long), c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    c->acc_pending = false;
    return F2Q_OK;
}

// the clear a reset left pending, now: before anything but a storing k_reduce_slabs reads or writes acc_d
static int acc_ready(f2q_ctx *c)
{
    if (!c->acc_pending) return F2Q_OK;
    HIPC(c, hipMemsetAsync(c->acc_d, 0, c->acc_n * sizeof(unsigned long long), c->stream));
    c->acc_pending = false;
    return F2Q_OK;
}

extern "C" int f2q_create(const f2q_params *p, f2q_ctx **out)
{
    if (!p || !out) return fail(nullptr, F2Q_EINVAL, "null argument");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1)
        return fail(nullptr, F2Q_ENODEVICE, std::string("no HIP device: ") + hipGetErrorString(e));
    if (p->device < 0 || p->device >= ndev) return fail(nullptr, F2Q_EINVAL, "device ordinal out of range");
    if (p->mode != 0 && p->mode != 1) return fail(nullptr, F2Q_EINVAL, "mode must be 0 (C) or 1 (EC)");
    f2q_ctx *c = new f2q_ctx();
    c->prm = *p;
    for (int i = 0; i < p->n_upstream && i < F2Q_MAX_ITER; i++) c->up_s.push_back(p->upstream[i] ? p->upstream[i] : "");
    for (int i = 0; i < p->n_downstream && i < F2Q_MAX_ITER; i++) c->down_s.push_back(p->downstream[i] ? p->downstream[i] : "");
    c->device = p->device;
    { const char *fv = getenv("F2Q_FORCE_V1"); c->force_v1 = fv && fv[0] == '1'; }
    { const char *tr = getenv("F2Q_TRACE"); c->trace = tr && tr[0] == '1'; }
    { const char *tr = getenv("F2Q_TRACE_SYNC"); c->trace_sync = tr && tr[0] == '1'; }
    { const char *dc = getenv("F2Q_DEV_CACHE_MB"); if (dc && atol(dc) >= 0) c->dev_idle_cap = (size_t)atol(dc) << 20; }
    { const char *fv = getenv("F2Q_GENERIC"); c->force_generic = fv && fv[0] == '1'; }
    { const char *fv = getenv("F2Q_NO_LT"); c->no_lt = fv && fv[0] == '1'; }
    { const char *fv = getenv("F2Q_LT_WGS"); if (fv && atoi(fv) > 0) c->lt_max_wgs = (uint32_t)atoi(fv); }
    { const char *fv = getenv("F2Q_NO_HOT"); c->no_hot = fv && fv[0] == '1'; }
    { const char *fv = getenv("F2Q_NO_PT"); c->no_pt = fv && fv[0] == '1'; }
    { const char *fv = getenv("F2Q_PT_PARTS"); if (fv && atoi(fv) > 0) c->ix.pt_force_parts = std::min(atoi(fv), (int)F2Q_PT_MAXP); }
    { const char *fv = getenv("F2Q_PT_CHUNK"); if (fv && atol(fv) > 0) c->pt_chunk_reads = (uint64_t)atol(fv); }
    { const char *fv = getenv("F2Q_PT_MIN_READS"); if (fv && atol(fv) >= 0) c->pt_min_reads = (uint64_t)atol(fv); }
    { const char *fv = getenv("F2Q_HOT_LEARN"); if (fv && atol(fv) > 0) c->hot_learn = (uint64_t)atol(fv); }
    { const char *fv = getenv("F2Q_HOST_PACK"); c->host_pack = fv && fv[0] == '1'; }
    { const char *fv = getenv("F2Q_FORCE_GENERAL"); c->force_general = fv && fv[0] == '1'; }
    int rc = setup_run(c);
    if (rc) { g_create_err = c->err; delete c; return rc; }
#define CREATE_HIP(call)                                                                            \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            g_create_err = std::string(#call) + ": " + hipGetErrorString(e_);                       \
            f2q_destroy(c);                                                                         \
            return F2Q_EHIP;                                                                        \
        }                                                                                           \
    } while (0)
    CREATE_HIP(hipSetDevice(c->device));
    hipDeviceProp_t prop;
    CREATE_HIP(hipGetDeviceProperties(&prop, c->device));
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    CREATE_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    CREATE_HIP(hipEventCreate(&c->ev_a)); CREATE_HIP(hipEventCreate(&c->ev_b));
    CREATE_HIP(hipEventCreate(&c->ev_k0)); CREATE_HIP(hipEventCreate(&c->ev_k1));
    CREATE_HIP(hipMalloc((void **)&c->run_d, sizeof(RunDev)));
    CREATE_HIP(hipMemcpyAsync(c->run_d, &c->run_h, sizeof(RunDev), hipMemcpyHostToDevice, c->stream));
    // an empty library so that EC mode (and a Counter run before set_features fails cleanly) has valid pointers
    build_index(c->ix, "", (const uint32_t[]){0}, 0, c->run_h.miss, 0);
    rc = upload_lib(c);
    if (!rc) rc = alloc_acc(c, 0);
    if (rc) { g_create_err = c->err; f2q_destroy(c); return rc; }
    *out = c;
    return F2Q_OK;
}

// the (feature, UMI) set given back: f2q_destroy, and a new library (umis[] has a word per feature)
static void pairset_drop(f2q_ctx *c, PairSet &s)
{
    free_all(c, s.set_allocs);
    s.dev->slots = nullptr; s.dev->reads = nullptr; s.n_slots = 0; s.held_ub = 0;
}
static void umi_drop(f2q_ctx *c)
{
    pairset_drop(c, c->umi.set); free_all(c, c->umi.fix_allocs);
    c->umi.dev.umis = nullptr; c->umi.dev.ctr = nullptr;
}

// the set and its counters (which the owner has allocated) cleared, the set's size kept
static int pairset_clear(f2q_ctx *c, PairSet &s)
{
    if (s.dev->slots) HIPC(c, hipMemsetAsync(s.dev->slots, 0xFF, s.n_slots * sizeof(unsigned long long), c->stream));
    if (s.dev->reads) HIPC(c, hipMemsetAsync(s.dev->reads, 0, s.n_slots * sizeof(uint32_t), c->stream));
    HIPC(c, hipMemsetAsync(s.dev->ctr, 0, F2Q_UMI_CTR_WORDS * sizeof(unsigned long long), c->stream));
    s.held_ub = 0;
    return F2Q_OK;
}
// the set, umis[] and the counters cleared (f2q_reset_counts)
static int umi_clear(f2q_ctx *c)
{
    HIPC(c, hipMemsetAsync(c->umi.dev.umis, 0, std::max<uint64_t>(c->lib_h.n_features, 1) * sizeof(unsigned long long), c->stream));
    return pairset_clear(c, c->umi.set);
}

// the set's counters after everything on the stream (all zero before the first launch); waits for the stream
static int pairset_read_ctr(f2q_ctx *c, const PairSet &s, unsigned long long ctr[F2Q_UMI_CTR_WORDS])
{
    for (int i = 0; i < F2Q_UMI_CTR_WORDS; i++) ctr[i] = 0;
    if (s.dev->ctr) HIPC(c, hipMemcpyAsync(ctr, s.dev->ctr, F2Q_UMI_CTR_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    if (ctr[F2Q_UMI_OVERFLOW]) return fail(c, F2Q_EHIP, std::string(s.name) + " set overflow (internal sizing error)");
    return F2Q_OK;
}
static void pairset_trace(const f2q_ctx *c, const PairSet &s)
{
    if (c->trace) fprintf(stderr, "[f2q trace] %s set: %llu slots, %llu rehashes\n", s.name, (unsigned long long)s.n_slots, (unsigned long long)s.rehashes);
}

// the barcode table, the matrix and the counters given back: f2q_destroy, and a new library
static void demux_drop(f2q_ctx *c)
{
    free_all(c, c->demux.allocs);
    c->demux.dev.table = nullptr; c->demux.dev.matrix = nullptr; c->demux.dev.sstats = nullptr; c->demux.dev.verdicts = nullptr; c->demux.matrix_n = 0;
}

// Table, matrix and counters once barcodes and features are both known, through the context's device-memory cache.  A
// failure gives back what this call got and leaves the context as it was: the call that led here may simply be repeated.
static int demux_alloc(f2q_ctx *c)
{
    if (c->demux.dev.matrix) return F2Q_OK;
    DemuxDev d = c->demux.dev; std::vector<void *> owner;
    const uint64_t nf = std::max<uint64_t>(c->lib_h.n_features, 1), rows = (uint64_t)d.n + 1;
    unsigned long long *tab = nullptr, *ctr = nullptr;
    int rc;
    if ((rc = dev_upload(c, (const unsigned long long *)c->demux.tab.slots.data(), c->demux.tab.slots.size(), &tab, owner)) ||
        (rc = dev_alloc(c, (size_t)(rows * nf), &d.matrix, owner, 0)) ||
        (rc = dev_alloc(c, (size_t)(rows * 5 + 5), &ctr, owner, 0))) {
        free_all(c, owner);
        return fail(c, F2Q_ENOMEM, "no device memory for the demultiplexed counts (" + std::to_string(rows) + " x " + std::to_string(nf) + " counters): " + c->err);
    }
    d.table = tab; d.sstats = ctr; d.verdicts = ctr + rows * 5; d.n_features = (uint32_t)c->lib_h.n_features;
    c->demux.dev = d; c->demux.allocs = owner; c->demux.matrix_n = rows * nf;
    return F2Q_OK;
}

// matrix and counters cleared (f2q_reset_counts); the table stays
static int demux_clear(f2q_ctx *c)
{
    HIPC(c, hipMemsetAsync(c->demux.dev.matrix, 0, c->demux.matrix_n * sizeof(unsigned long long), c->stream));
    HIPC(c, hipMemsetAsync(c->demux.dev.sstats, 0, ((size_t)c->demux.dev.n + 2) * 5 * sizeof(unsigned long long), c->stream));
    return F2Q_OK;
}

// the reverse-strand counts and the strand counters given back: f2q_destroy, and a new library
static void strand_drop(f2q_ctx *c)
{
    free_all(c, c->strand.allocs);
    c->strand.dev.rev_counts = nullptr; c->strand.dev.extra = nullptr; c->strand.words = 0;
}

// rev_counts and the four counters once the mode and the features are both known, zeroed.  A failure leaves the context as
// it was: the call that led here may simply be repeated.
static int strand_alloc(f2q_ctx *c)
{
    if (c->strand.dev.rev_counts) return F2Q_OK;
    const uint64_t nf = std::max<uint64_t>(c->lib_h.n_features, 1);
    unsigned long long *w = nullptr; std::vector<void *> owner;
    if (dev_alloc(c, (size_t)(nf + 4), &w, owner, 0)) {
        free_all(c, owner);
        return fail(c, F2Q_ENOMEM, "no device memory for the reverse-strand counts (" + std::to_string(nf) + " counters): " + c->err);
    }
    c->strand.dev.rev_counts = w; c->strand.dev.extra = w + nf; c->strand.allocs = owner; c->strand.words = nf + 4;
    return F2Q_OK;
}

// ---- one-base insertions and deletions: the variant table and the counters -----------------------------------------------
static void indel_drop(f2q_ctx *c)
{
    free_all(c, c->indel.allocs);
    c->indel.dev = IndelDev{}; c->indel.words = 0;
}

// The deletion-variant table of the context's library and zeroed counters, built next to what the context holds and
// swapped in at the end: a failure leaves the context as it was.  Without a library there is nothing to build yet.
static int indel_install(f2q_ctx *c, bool lib_known)
{
    if (!lib_known) return F2Q_OK;
    const int L = c->run_h.length;
    const uint64_t nf = std::max<uint64_t>(c->ix.n_features, 1);
    if ((uint64_t)c->ix.grp[L].n * (uint64_t)L > 0x40000000ull) return fail(c, F2Q_ENOMEM, "f2q_set_indel: the deletion-variant table of " + std::to_string(c->ix.grp[L].n) + " features is not built");
    IndelTable t;
    indel_build(c->ix, L, t);
    std::vector<void *> owner; IndelDev d{};
    uint64_t *keys = nullptr, *vals = nullptr; unsigned long long *w = nullptr;
    const uint64_t words = 2 * nf + 2 * (uint64_t)L + F2Q_INDEL_TOTALS;
    if (dev_upload(c, t.keys.data(), t.keys.size(), &keys, owner) || dev_upload(c, t.vals.data(), t.vals.size(), &vals, owner) ||
        dev_alloc(c, (size_t)words, &w, owner, 0)) {
        free_all(c, owner);
        return fail(c, F2Q_ENOMEM, "no device memory for the deletion-variant table (" + std::to_string(t.keys.size()) + " slots) and the indel counters: " + c->err);
    }
    HIPC(c, hipStreamSynchronize(c->stream));                    // (the uploads read t)
    indel_drop(c);
    d.var_keys = keys; d.var_vals = vals; d.var_bits = t.bits;
    d.del_counts = w; d.ins_counts = w + nf; d.del_pos = w + 2 * nf; d.ins_pos = w + 2 * nf + L; d.totals = w + 2 * nf + 2 * L;
    c->indel.dev = d; c->indel.allocs = owner; c->indel.words = words;
    if (c->trace) fprintf(stderr, "[f2q trace] indel: every read takes k_count_indel; deletion-variant table %zu slots (%llu variants of %llu candidates, %llu shared)\n",
                          t.keys.size(), (unsigned long long)t.variants, (unsigned long long)t.candidates, (unsigned long long)t.shared);
    return F2Q_OK;
}

// ---- pair libraries, each part matched alone: tables, counters and the recombinant set ---------------------------------
// everything given back: f2q_destroy, and a new library
static void parts_drop(f2q_ctx *c)
{
    for (int k = 0; k < 2; k++) free_all(c, c->parts.lib_allocs[k]);
    free_all(c, c->parts.fix_allocs); pairset_drop(c, c->parts.set);
    c->parts.dev = PartsDev{}; c->parts.words = 0;
}

// The part libraries, the pair table and zeroed counters for the library seqs / offs / n (f2q_set_features' arguments),
// built next to what the context holds and swapped in at the end: a failure (F2Q_EINVAL: a feature that is not two parts,
// named in the message; F2Q_ENOMEM) leaves the context as it was.  The set starts empty (pairset_reserve allocates it).
static int parts_install(f2q_ctx *c, const char *seqs, const uint32_t *offs, uint32_t n)
{
    PartsTable t; std::string err;
    if (int rc = parts_validate(seqs, offs, n, t, err)) return fail(c, rc, "f2q_set_parts: " + err);
    parts_build(t);
    HostIndex ix[2]; LibDev lh[2]; LibDev *ld[2] = {nullptr, nullptr}; std::vector<void *> la[2], fix;
    PartsDev d{};
    unsigned long long *keys = nullptr, *words = nullptr, *ctr = nullptr; uint32_t *feat = nullptr, *ids = nullptr;
    const uint64_t nf = std::max<uint64_t>(n, 1), n1 = std::max<uint64_t>(t.n(0), 1), n2 = std::max<uint64_t>(t.n(1), 1);
    int rc = F2Q_OK;
    for (int k = 0; k < 2 && !rc; k++) {
        build_index(ix[k], t.seqs[k].data(), t.offs[k].data(), t.n(k), c->run_h.miss, 0);
        rc = upload_index(c, ix[k], lh[k], &ld[k], la[k], nullptr);
    }
    if (rc || (rc = dev_upload(c, (const unsigned long long *)t.keys.data(), t.keys.size(), &keys, fix)) ||
        (rc = dev_upload(c, t.feat.data(), t.feat.size(), &feat, fix)) || (rc = dev_upload(c, t.ids.data(), t.ids.size(), &ids, fix)) ||
        (rc = dev_alloc(c, (size_t)(nf + n1 + n2 + F2Q_PARTS_CLASSES), &words, fix, 0)) ||
        (rc = dev_alloc(c, (size_t)F2Q_UMI_CTR_WORDS, &ctr, fix, 0))) {
        for (int k = 0; k < 2; k++) free_all(c, la[k]);
        free_all(c, fix);
        return fail(c, F2Q_ENOMEM, "no device memory for the part libraries and tables (" + std::to_string(n1) + " + " + std::to_string(n2) + " parts, " + std::to_string(nf) + " features): " + c->err);
    }
    HIPC(c, hipStreamSynchronize(c->stream));                    // (the uploads read t, which moves below)
    parts_drop(c);
    d.lib1 = ld[0]; d.lib2 = ld[1]; d.pair_keys = keys; d.pair_feat = feat; d.pair_mask = t.mask; d.n_features = n; d.ids = ids;
    d.counts = words; d.part1 = words + nf; d.part2 = words + nf + n1; d.classes = words + nf + n1 + n2;
    d.rec.ctr = ctr;
    c->parts.dev = d; c->parts.words = nf + n1 + n2 + F2Q_PARTS_CLASSES; c->parts.fix_allocs = fix;
    for (int k = 0; k < 2; k++) { c->parts.ix[k] = std::move(ix[k]); c->parts.lib_h[k] = lh[k]; c->parts.lib_allocs[k] = la[k]; }
    c->parts.tab = std::move(t);
    if (c->trace) fprintf(stderr, "[f2q trace] parts: n1 %u, n2 %u, pair table %zu slots (%u pairs of %u features)\n",
                          c->parts.tab.n(0), c->parts.tab.n(1), c->parts.tab.keys.size(), c->parts.tab.pairs, n);
    return F2Q_OK;
}

// counters and the set cleared (f2q_reset_counts); the tables and the set's size stay
static int parts_clear(f2q_ctx *c)
{
    HIPC(c, hipMemsetAsync(c->parts.dev.counts, 0, c->parts.words * sizeof(unsigned long long), c->stream));
    return pairset_clear(c, c->parts.set);
}

// ---- the raw-record modes: one life cycle ---------------------------------------------------------------------------------
// f2q_set_features has a new library in place (seqs / offs / n: its arguments): what the mode holds per feature starts afresh
static int mode_on_library(f2q_ctx *c, const char *seqs, const uint32_t *offs, uint32_t n)
{
    switch (c->raw_mode) {
        case RAW_NONE:    break;
        case RAW_UMI:     umi_drop(c); break;                             // a new set; umis[] has a word per feature
        case RAW_DEMUX:   demux_drop(c); return demux_alloc(c);           // a new matrix: a row has a word per feature
        case RAW_STRAND:  strand_drop(c); return strand_alloc(c);
        case RAW_STAGGER: HIPC(c, hipMemsetAsync(c->stagger.dev.hist, 0, 2 * ((size_t)c->stagger.n + 1) * sizeof(unsigned long long), c->stream)); break;
        case RAW_INDEL:   return indel_install(c, true);                  // a variant table and indel counters of its own
        case RAW_PARTS:   return parts_install(c, seqs, offs, n);         // part libraries, a pair table and a set of its own
    }
    return F2Q_OK;
}
// f2q_reset_counts: what the mode has counted cleared, tables and sizes kept (nothing to clear before the first allocation)
static int mode_clear(f2q_ctx *c)
{
    switch (c->raw_mode) {
        case RAW_NONE:    break;
        case RAW_UMI:     if (c->umi.dev.umis) return umi_clear(c); break;
        case RAW_DEMUX:   if (c->demux.dev.matrix) return demux_clear(c); break;
        case RAW_STRAND:  if (c->strand.dev.rev_counts) HIPC(c, hipMemsetAsync(c->strand.dev.rev_counts, 0, c->strand.words * sizeof(unsigned long long), c->stream)); break;
        case RAW_STAGGER: HIPC(c, hipMemsetAsync(c->stagger.dev.hist, 0, 2 * ((size_t)c->stagger.n + 1) * sizeof(unsigned long long), c->stream)); break;
        case RAW_INDEL:   if (c->indel.dev.del_counts) HIPC(c, hipMemsetAsync(c->indel.dev.del_counts, 0, c->indel.words * sizeof(unsigned long long), c->stream)); break;
        case RAW_PARTS:   if (c->parts.dev.counts) return parts_clear(c); break;
    }
    return F2Q_OK;
}
// everything the mode holds given back: f2q_destroy (the two pair sets say how far they grew: F2Q_TRACE), and a stagger or
// an indel context that becomes a plain one again.  No other mode holds device memory.
static void mode_drop(f2q_ctx *c)
{
    switch (c->raw_mode) {
        case RAW_NONE:    break;
        case RAW_UMI:     pairset_trace(c, c->umi.set); umi_drop(c); break;
        case RAW_DEMUX:   demux_drop(c); break;
        case RAW_STRAND:  strand_drop(c); break;
        case RAW_STAGGER: free_all(c, c->stagger.allocs); c->stagger.n = 0; c->stagger.dev = StaggerDev{}; break;
        case RAW_INDEL:   indel_drop(c); break;
        case RAW_PARTS:   pairset_trace(c, c->parts.set); parts_drop(c); break;
    }
}

extern "C" void f2q_destroy(f2q_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->trace) fprintf(stderr, "[f2q trace] device memory: %llu hipMalloc %.1f ms, %llu hipFree %.1f ms, %llu reused; Extract+Count reserve %.1f ms (%llu rehashes)\n",
                          (unsigned long long)c->n_malloc, c->tr_malloc, (unsigned long long)c->n_hipfree, c->tr_hipfree, (unsigned long long)c->n_reuse, c->tr_reserve, (unsigned long long)c->n_rehash);
    if (c->aux_stream) (void)hipStreamSynchronize(c->aux_stream);
    free_all(c, c->lib_allocs); free_all(c, c->ec_allocs); free_all(c, c->ec_allocs64); free_all(c, c->ec_allocs_ctr); free_all(c, c->hot_allocs);
    free_all(c, c->asg_lib_allocs); free_all(c, c->asg_allocs); free_all(c, c->ecc_allocs);
    mode_drop(c);
    if (c->asg_acc_d) (void)hipFree(c->asg_acc_d);
    if (c->defer_d) (void)hipFree(c->defer_d);
    for (auto &kv : c->dev_idle) (void)hipFree(kv.second);
    c->dev_idle.clear(); c->dev_size.clear();
    if (c->acc_d) (void)hipFree(c->acc_d);
    if (c->carry_d) (void)hipFree(c->carry_d);
    if (c->synth_keys_d) (void)hipFree(c->synth_keys_d);
    if (c->slab_d) (void)hipFree(c->slab_d);
    if (c->stat_slab_d) (void)hipFree(c->stat_slab_d);
    if (c->hit_buf_d) (void)hipFree(c->hit_buf_d);
    if (c->pt_s.streams) (void)hipFree(c->pt_s.streams);
    if (c->pt_s.cnt) (void)hipFree(c->pt_s.cnt);
    if (c->pt_stat_d) (void)hipFree(c->pt_stat_d);
    if (c->pt_slab0_d) (void)hipFree(c->pt_slab0_d);
    if (c->pt_slab1_d) (void)hipFree(c->pt_slab1_d);
    if (c->run_d) (void)hipFree(c->run_d);
    if (c->ev_a) (void)hipEventDestroy(c->ev_a);
    if (c->ev_b) (void)hipEventDestroy(c->ev_b);
    if (c->ev_k0) (void)hipEventDestroy(c->ev_k0);
    if (c->ev_k1) (void)hipEventDestroy(c->ev_k1);
    for (hipEvent_t e : c->q_ev) (void)hipEventDestroy(e);
    if (c->ev_copy) (void)hipEventDestroy(c->ev_copy);
    if (c->ev_aux0) (void)hipEventDestroy(c->ev_aux0);
    if (c->ev_aux1) (void)hipEventDestroy(c->ev_aux1);
    if (c->aux_stream) (void)hipStreamDestroy(c->aux_stream);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

extern "C" int f2q_set_features(f2q_ctx *c, const char *seqs, const uint32_t *offs, uint32_t n)
{
    if (!c || !offs || (!seqs && n)) return fail(c, F2Q_EINVAL, "null argument");
    if (c->prm.mode != 0) return fail(c, F2Q_ESTATE, "Extract+Count mode takes no feature library (fast2q.py:1701)");
    HIPC(c, hipSetDevice(c->device));
    for (uint32_t i = 0; i < n; i++) if (offs[i + 1] < offs[i]) return fail(c, F2Q_EINVAL, "offsets must be non-decreasing");
    if (c->raw_mode == RAW_PARTS) {                   // a parts context takes A:B libraries only: refused before anything changes
        PartsTable t; std::string err;
        if (int rc = parts_validate(seqs ? seqs : "", offs, n, t, err)) return fail(c, rc, "f2q_set_features on a parts context (f2q_set_parts): " + err);
    }
    c->plan = make_plan(c->run_h);                   // the library decides below whether the packed paths apply
    c->plan.rc2 = c->rc2;
    if (c->force_general) { c->plan.fast_fixed = false; c->plan.fast_anchor = false; c->plan.multi = false; c->plan.multi_pair = false; }
    int packed_len = c->plan.fast_fixed ? c->run_h.length : 0;
    if (c->plan.fast_anchor) {
        if (c->run_h.has_up && c->run_h.has_down) {          // variable windows: index the most common feature length
            std::vector<uint32_t> hist(F2Q_REG_MAXLEN + 1, 0);
            for (uint32_t i = 0; i < n; i++) { uint32_t l = offs[i + 1] - offs[i]; if (l >= 1 && l <= F2Q_REG_MAXLEN) hist[l]++; }
            packed_len = (int)(std::max_element(hist.begin(), hist.end()) - hist.begin());
        } else packed_len = c->run_h.length;
    }
    build_index(c->ix, seqs ? seqs : "", offs, n, c->run_h.miss, packed_len, c->plan.multi ? c->run_h.n_iter : 0);
    // multi-window runs stay on the packed path only when every reachable feature is a k-part feature
    if (c->plan.multi && (!c->ix.mw_ok || c->ix.n_irregular)) { c->plan.multi = false; c->plan.fast_fixed = false; }
    int rc = upload_lib(c);
    if (rc) return rc;
    rc = alloc_acc(c, n);
    if (rc) return rc;
    if ((rc = mode_on_library(c, seqs ? seqs : "", offs, n))) return rc;
    c->plan.inband_n = (c->plan.fast_fixed || c->plan.fast_anchor) && c->ix.n_irregular == 0;
    // two pairs against a pure A:B library (pair tables): an 'N' travels as a flag bit (a forced mismatch; it equals no
    // symbol of any feature), every other odd symbol still sends the read to the byte-exact routine
    if (c->plan.fast_anchor && c->plan.multi_pair && c->prm.mode == 0 && c->run_h.n_iter == 2 && c->lib_h.pw.ok) { c->plan.inband_n = true; c->plan.n_only = true; }
    if (c->ix.n_irregular && !c->plan.multi_pair) c->plan.fast_anchor = false;      // irregular features need the byte-exact routine (the pair kernel matches strings)
    c->have_lib = true;
    return F2Q_OK;
}

extern "C" int f2q_reset_counts(f2q_ctx *c)
{
    if (!c) return F2Q_EINVAL;
    HIPC(c, hipSetDevice(c->device));
    // the accumulators are cleared by whoever touches them next: a storing k_reduce_slabs, which needs no clear at all, or
    // acc_ready.  A context whose raw pointer is out clears here and now
    c->acc_pending = true;
    if (c->acc_eager) if (int rc = acc_ready(c)) return rc;
    if (c->prm.mode == 1) {
        if (c->aux_stream) HIPC(c, hipStreamSynchronize(c->aux_stream));
        c->aux_busy = false;
        free_all(c, c->ec_allocs); free_all(c, c->ec_allocs64); free_all(c, c->ec_allocs_ctr);
        memset(&c->ec, 0, sizeof c->ec); c->ec_slots = 0; c->hot_valid = false; c->ec_learned = 0;
    }
    if (int rc = mode_clear(c)) return rc;
    c->reads_seen = 0;
    c->ec_gen++;
    // no host synchronisation: the clear is ordered on the context's stream like every launch and read-back after it
    return F2Q_OK;
}

extern "C" int f2q_set_read_base(f2q_ctx *c, uint64_t first_read_index)
{
    if (!c) return F2Q_EINVAL;
    c->reads_seen = first_read_index;
    return F2Q_OK;
}

extern "C" int f2q_read_counts(f2q_ctx *c, int64_t *counts, int64_t stats[5])
{
    if (!c) return F2Q_EINVAL;
    HIPC(c, hipSetDevice(c->device));
    if (int rc = acc_ready(c)) return rc;
    std::vector<unsigned long long> h(c->acc_n);
    HIPC(c, hipMemcpyAsync(h.data(), c->acc_d, c->acc_n * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    if (counts) for (uint64_t i = 0; i + 5 < c->acc_n; i++) counts[i] = (int64_t)h[i];
    if (stats) for (int k = 0; k < 5; k++) stats[k] = (int64_t)h[c->acc_n - 5 + k];
    return F2Q_OK;
}

extern "C" int f2q_counts_device_ptr(f2q_ctx *c, void **dptr, uint64_t *n_int64)
{
    if (!c || !dptr || !n_int64) return F2Q_EINVAL;
    HIPC(c, hipSetDevice(c->device));
    if (int rc = acc_ready(c)) return rc;            // (queued on the stream, as the reset's own clear used to be)
    c->acc_eager = true;
    *dptr = c->acc_d; *n_int64 = c->acc_n;
    return F2Q_OK;
}

// ---- distinct UMIs per feature: the ABI ---------------------------------------------------------------------------
// what the three UMI setters share once the window is in umi.dev
static void umi_enable(f2q_ctx *c)
{
    c->umi.set.min_slots = pairset_min_slots_from_env("F2Q_UMI_SLOTS");
    raw_road_enter(c, RAW_UMI);
}
extern "C" int f2q_set_umi(f2q_ctx *c, int32_t start, int32_t length)
{
    if (!c) return F2Q_EINVAL;
    if (int rc = raw_mode_enter(c, RAW_UMI, "f2q_set_umi", c->n_mate1 ? "takes single reads: a paired context (f2q_set_mate2) takes f2q_set_umi_paired" : "")) return rc;
    if (start < 0 || start > 0x3FFFFFFF || length < 1 || length > F2Q_UMI_MAXLEN)
        return fail(c, F2Q_EINVAL, "the UMI window needs a start >= 0 and a length of 1 .. 16 bases");
    c->umi.dev.start = start; c->umi.dev.length = length;
    umi_enable(c);
    return F2Q_OK;
}

// The UMI in the read header (include/f2q.h): the last `sep`-separated field of the read id, `length` bases.  On a paired
// context the header is mate 1's.  The ingest drivers run k_header_umi on the framed text (the host twin: header_umis) and
// the block carries the result; the counting kernels are the HDR instances of k_count_umi / k_count_umi_pair.
extern "C" int f2q_set_umi_header(f2q_ctx *c, int32_t sep, int32_t length)
{
    if (!c) return F2Q_EINVAL;
    if (int rc = raw_mode_enter(c, RAW_UMI, "f2q_set_umi_header")) return rc;
    const bool alnum = (sep >= '0' && sep <= '9') || (sep >= 'A' && sep <= 'Z') || (sep >= 'a' && sep <= 'z');
    if (sep < 33 || sep > 126 || alnum || sep == '+' || length < 1 || length > F2Q_UMI_MAXLEN)
        return fail(c, F2Q_EINVAL, "the header UMI needs a separator that is one printable ASCII byte (33 .. 126), not alphanumeric and not '+', and a length of 1 .. 16 bases");
    UmiDev &u = c->umi.dev;
    u.start = 0; u.length = length; u.start1 = u.len1 = u.start2 = u.len2 = 0; u.rc2 = c->rc2 ? 1 : 0;
    c->umi.hdr_sep = sep;
    umi_enable(c);
    return F2Q_OK;
}

// The UMI of a pair: [start1, start1 + length1) of mate 1 followed by [start2, start2 + length2) of mate 2 as sequenced
// (include/f2q.h).  The context stays paired in every other respect: the ingest kernels see a plan without fast paths, so
// read_is_clean is false for every pair and all of them travel as merged raw records to k_count_umi_pair.
extern "C" int f2q_set_umi_paired(f2q_ctx *c, int32_t start1, int32_t length1, int32_t start2, int32_t length2)
{
    if (!c) return F2Q_EINVAL;
    // (a single-read context with another mode in place hears of the mode: the want of a second mate comes after)
    if (int rc = raw_mode_enter(c, RAW_UMI, "f2q_set_umi_paired")) return rc;
    if (!c->n_mate1) return fail(c, F2Q_ESTATE, "f2q_set_umi_paired takes a paired context: call f2q_set_mate2 first (single reads: f2q_set_umi)");
    if (start1 < 0 || start1 > 0x3FFFFFFF || start2 < 0 || start2 > 0x3FFFFFFF || length1 < 0 || length2 < 0 ||
        length1 > F2Q_UMI_MAXLEN || length2 > F2Q_UMI_MAXLEN || length1 + length2 < 1 || length1 + length2 > F2Q_UMI_MAXLEN)
        return fail(c, F2Q_EINVAL, "the UMI parts need starts >= 0 and lengths >= 0 that add up to 1 .. 16 bases");
    UmiDev &u = c->umi.dev;
    u.start = 0; u.length = length1 + length2;
    u.start1 = length1 ? start1 : 0; u.len1 = length1; u.start2 = length2 ? start2 : 0; u.len2 = length2; u.rc2 = c->rc2 ? 1 : 0;
    // F2Q_UMI_PAIR_STAGE=1 / 0: the merged lines staged in LDS / read from global memory (A/B runs; the default: DESIGN.md)
    { const char *e = getenv("F2Q_UMI_PAIR_STAGE"); c->umi.pair_stage = e && (e[0] == '0' || e[0] == '1') && !e[1] ? e[0] == '1' : F2Q_UMI_PAIR_STAGE_DEFAULT; }
    umi_enable(c);
    return F2Q_OK;
}

extern "C" int f2q_set_umi_reads(f2q_ctx *c, int32_t on)
{
    if (!c) return F2Q_EINVAL;
    if (c->raw_mode != RAW_UMI) return fail(c, F2Q_ESTATE, "not a UMI context: call f2q_set_umi first");
    if (c->counted) return fail(c, F2Q_ESTATE, "f2q_set_umi_reads comes after f2q_set_umi and before counting");
    c->umi.set.keep_reads = on != 0;
    return F2Q_OK;
}

extern "C" int f2q_read_umis(f2q_ctx *c, int64_t *umis, int64_t extra[2])
{
    if (!c) return F2Q_EINVAL;
    if (c->raw_mode != RAW_UMI) return fail(c, F2Q_ESTATE, "not a UMI context: call f2q_set_umi first");
    HIPC(c, hipSetDevice(c->device));
    const uint64_t nf = c->lib_h.n_features;
    std::vector<unsigned long long> h(nf, 0ull);
    unsigned long long ctr[F2Q_UMI_CTR_WORDS];
    if (c->umi.dev.umis && nf)                                   // (nothing counted yet: all zero)
        HIPC(c, hipMemcpyAsync(h.data(), c->umi.dev.umis, nf * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    if (int rc = pairset_read_ctr(c, c->umi.set, ctr)) return rc;
    if (umis) for (uint64_t i = 0; i < nf; i++) umis[i] = (int64_t)h[i];
    if (extra) { extra[0] = (int64_t)ctr[F2Q_UMI_READS]; extra[1] = (int64_t)ctr[F2Q_UMI_FAILED]; }
    return F2Q_OK;
}

// ---- inline sample barcodes: the ABI (include/f2q.h) -----------------------------------------------------------------
extern "C" int f2q_set_sample_barcodes(f2q_ctx *c, const char *seqs, uint32_t n, int32_t length, int32_t start, int32_t miss)
{
    if (!c) return F2Q_EINVAL;
    if (int rc = raw_mode_enter(c, RAW_DEMUX, "f2q_set_sample_barcodes")) return rc;
    std::string up, err;
    if (int rc = demux_validate(seqs, n, length, start, miss, up, err)) return fail(c, rc, err);
    HIPC(c, hipSetDevice(c->device));
    demux_build(up, n, length, miss, c->demux.tab);
    DemuxDev &d = c->demux.dev;
    d = DemuxDev{};
    d.mask = c->demux.tab.mask; d.start = start; d.length = length; d.miss = miss; d.n = n;
    // F2Q_DEMUX_TABLE=lds / global: the table copied into LDS by every workgroup (when it fits) / read from global memory
    const char *e = getenv("F2Q_DEMUX_TABLE");
    const bool want_lds = e && !strcmp(e, "lds") ? true : e && !strcmp(e, "global") ? false : F2Q_DEMUX_TABLE_LDS_DEFAULT;
    c->demux.lds_table = want_lds && c->demux.tab.slots.size() <= F2Q_DEMUX_LDS_SLOTS;
    if (c->have_lib) if (int rc = demux_alloc(c)) return rc;     // (the mode is not in place: as if the call had not been made)
    raw_road_enter(c, RAW_DEMUX);
    if (c->trace) fprintf(stderr, "[f2q trace] sample barcodes: %u of %d bases at %d, %d mismatches; table %zu slots, %u entries, %u ambiguous, %s\n",
                          n, length, start, miss, c->demux.tab.slots.size(), c->demux.tab.entries, c->demux.tab.ambiguous, c->demux.lds_table ? "LDS" : "global");
    return F2Q_OK;
}

extern "C" int f2q_read_demux(f2q_ctx *c, int64_t *matrix, int64_t *sample_stats, int64_t verdicts[5])
{
    if (!c) return F2Q_EINVAL;
    if (c->raw_mode != RAW_DEMUX) return fail(c, F2Q_ESTATE, "not a demultiplexing context: call f2q_set_sample_barcodes first");
    HIPC(c, hipSetDevice(c->device));
    const DemuxDev &d = c->demux.dev;
    const uint64_t nf = c->have_lib ? c->lib_h.n_features : 0, rows = (uint64_t)d.n + 1;
    std::vector<unsigned long long> hm, hs(rows * 5 + 5, 0ull);
    if (d.matrix) {                                              // (no library yet: nothing can have been counted)
        if (matrix && nf) {
            try { hm.resize(rows * nf); } catch (const std::bad_alloc &) { return fail(c, F2Q_ENOMEM, "no host memory to copy the demultiplexed counts"); }
            HIPC(c, hipMemcpyAsync(hm.data(), d.matrix, rows * nf * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        }
        HIPC(c, hipMemcpyAsync(hs.data(), d.sstats, hs.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    }
    HIPC(c, hipStreamSynchronize(c->stream));
    if (matrix) for (uint64_t i = 0; i < rows * nf; i++) matrix[i] = hm.empty() ? 0 : (int64_t)hm[i];
    if (sample_stats) for (uint64_t i = 0; i < rows * 5; i++) sample_stats[i] = (int64_t)hs[i];
    if (verdicts) for (int k = 0; k < 5; k++) verdicts[k] = (int64_t)hs[rows * 5 + k];
    return F2Q_OK;
}

// ---- read orientation: the ABI (include/f2q.h) ------------------------------------------------------------------------
extern "C" int f2q_set_strand(f2q_ctx *c, int32_t mode)
{
    if (!c) return F2Q_EINVAL;
    if (mode != F2Q_STRAND_FWD && mode != F2Q_STRAND_REV && mode != F2Q_STRAND_BOTH)
        return fail(c, F2Q_EINVAL, "the strand mode is F2Q_STRAND_FWD (0), F2Q_STRAND_REV (1) or F2Q_STRAND_BOTH (2), not " + std::to_string(mode));
    if (mode == F2Q_STRAND_FWD) return F2Q_OK;               // the record as written: what every context does
    if (int rc = raw_mode_enter(c, RAW_STRAND, "f2q_set_strand (rev / both)")) return rc;
    HIPC(c, hipSetDevice(c->device));
    c->strand.dev = StrandDev{}; c->strand.dev.mode = mode;
    if (c->have_lib) if (int rc = strand_alloc(c)) return rc;    // (the mode is not in place: as if the call had not been made)
    c->strand.mode = mode;
    raw_road_enter(c, RAW_STRAND);
    if (c->trace) fprintf(stderr, "[f2q trace] strand mode %s: every read takes k_count_strand<%s>\n", mode == F2Q_STRAND_BOTH ? "both" : "rev", mode == F2Q_STRAND_BOTH ? "true" : "false");
    return F2Q_OK;
}

extern "C" int f2q_read_strands(f2q_ctx *c, int64_t *rev_counts, int64_t extra[4])
{
    if (!c) return F2Q_EINVAL;
    if (c->raw_mode != RAW_STRAND) return fail(c, F2Q_ESTATE, "no strand mode: call f2q_set_strand with F2Q_STRAND_REV or F2Q_STRAND_BOTH first");
    HIPC(c, hipSetDevice(c->device));
    const uint64_t nf = c->have_lib ? c->lib_h.n_features : 0;
    std::vector<unsigned long long> h;
    if (c->strand.dev.rev_counts) {                          // (no library yet: nothing can have been counted)
        try { h.resize(c->strand.words); } catch (const std::bad_alloc &) { return fail(c, F2Q_ENOMEM, "no host memory to copy the reverse-strand counts"); }
        HIPC(c, hipMemcpyAsync(h.data(), c->strand.dev.rev_counts, c->strand.words * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    }
    HIPC(c, hipStreamSynchronize(c->stream));
    if (rev_counts) for (uint64_t f = 0; f < nf; f++) rev_counts[f] = h.empty() ? 0 : (int64_t)h[f];
    if (extra) for (int k = 0; k < 4; k++) extra[k] = h.empty() ? 0 : (int64_t)h[c->strand.words - 4 + k];
    return F2Q_OK;
}

// ---- staggered libraries: the ABI (include/f2q.h) ---------------------------------------------------------------------
// A stagger or an indel context becomes a plain one again: what the mode held goes back, F2Q_FORCE_GENERAL says again what
// it said, and the plan is what f2q_create and f2q_set_features would have made of it
static int raw_road_leave(f2q_ctx *c)
{
    mode_drop(c);
    c->raw_mode = RAW_NONE;
    c->force_general = c->env_general;
    if (!c->have_lib) return setup_run(c);
    const std::string bytes((const char *)c->ix.feat_bytes.data(), c->ix.feat_bytes.size());      // (build_index rewrites c->ix)
    const std::vector<uint32_t> offs(c->ix.feat_off.begin(), c->ix.feat_off.end());
    return f2q_set_features(c, bytes.data(), offs.data(), c->ix.n_features);
}

// the shape f2q_set_stagger and f2q_set_indel ask of the run: what is wrong with it, for raw_mode_enter ("" when nothing is)
static std::string one_fixed_window(const f2q_ctx *c)
{
    if (!c->run_h.fixed) return "takes a fixed window (--st): an anchored run (--us/--ds) finds its window itself";
    if (c->run_h.n_iter != 1) return "takes exactly one window (--st with one value), not " + std::to_string(c->run_h.n_iter);
    if (c->run_h.start[0] < 0) return "takes a window that starts at or after the first base (--st >= 0)";
    return "";
}

extern "C" int f2q_set_stagger(f2q_ctx *c, int32_t n)
{
    if (!c) return F2Q_EINVAL;
    if (n < 0 || n > F2Q_STAGGER_MAX) return fail(c, F2Q_EINVAL, "f2q_set_stagger takes 0 .. 32 extra starts, not " + std::to_string(n));
    if (n == 0 && c->raw_mode != RAW_STAGGER) return F2Q_OK; // a plain context stays one: accepted at any time
    if (c->counted) return fail(c, F2Q_ESTATE, "f2q_set_stagger comes before counting");
    if (n == 0) {                                            // a plain context again
        HIPC(c, hipSetDevice(c->device));
        return raw_road_leave(c);
    }
    if (int rc = raw_mode_enter(c, RAW_STAGGER, "f2q_set_stagger", one_fixed_window(c))) return rc;
    HIPC(c, hipSetDevice(c->device));
    unsigned long long *w = nullptr; std::vector<void *> owner;
    if (dev_alloc(c, 2 * ((size_t)n + 1), &w, owner, 0)) {
        free_all(c, owner);
        return fail(c, F2Q_ENOMEM, "no device memory for the offset histograms: " + c->err);
    }
    free_all(c, c->stagger.allocs);                          // (of an earlier call with another n)
    c->stagger.allocs = owner;
    c->stagger.n = n; c->stagger.dev.n = n; c->stagger.dev.hist = w;
    { const char *e = getenv("F2Q_STAGGER_WALK"); c->stagger.dev.walk = e && e[0] == '1'; }
    raw_road_enter(c, RAW_STAGGER);
    if (c->trace) fprintf(stderr, "[f2q trace] stagger %d: every read takes k_count_stagger (%s layout)\n", n, c->stagger.dev.walk ? "walk" : "span");
    return F2Q_OK;
}

extern "C" int f2q_read_stagger(f2q_ctx *c, int64_t *perfect, int64_t *imperfect, int32_t n_offsets)
{
    if (!c) return F2Q_EINVAL;
    if (c->raw_mode != RAW_STAGGER) return fail(c, F2Q_ESTATE, "not a stagger context: call f2q_set_stagger with 1 .. 32 first");
    if (n_offsets != c->stagger.n + 1) return fail(c, F2Q_EINVAL, "f2q_read_stagger takes n_offsets = n + 1 = " + std::to_string(c->stagger.n + 1) + ", not " + std::to_string(n_offsets));
    HIPC(c, hipSetDevice(c->device));
    unsigned long long h[2 * (F2Q_STAGGER_MAX + 1)];
    HIPC(c, hipMemcpyAsync(h, c->stagger.dev.hist, 2 * (size_t)n_offsets * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    for (int32_t d = 0; d < n_offsets; d++) {
        if (perfect) perfect[d] = (int64_t)h[d];
        if (imperfect) imperfect[d] = (int64_t)h[n_offsets + d];
    }
    return F2Q_OK;
}

// ---- one-base insertions and deletions: the ABI (include/f2q.h) ---------------------------------------------------------
extern "C" int f2q_set_indel(f2q_ctx *c, int32_t on)
{
    if (!c) return F2Q_EINVAL;
    if (!on && c->raw_mode != RAW_INDEL) return F2Q_OK;      // a plain context stays one: accepted at any time
    if (c->counted) return fail(c, F2Q_ESTATE, "f2q_set_indel comes before counting");
    if (!on) {                                               // a plain context again
        HIPC(c, hipSetDevice(c->device));
        return raw_road_leave(c);
    }
    if (c->raw_mode == RAW_INDEL) return F2Q_OK;
    std::string shape = one_fixed_window(c);
    if (shape.empty() && (c->run_h.length < 2 || c->run_h.length > F2Q_REG_MAXLEN)) shape = "takes a window length (--l) of 2 .. 31 bases, not " + std::to_string(c->run_h.length);
    if (int rc = raw_mode_enter(c, RAW_INDEL, "f2q_set_indel", shape)) return rc;
    HIPC(c, hipSetDevice(c->device));
    if (int rc = indel_install(c, c->have_lib)) return rc;       // (the mode is not in place: as if the call had not been made)
    raw_road_enter(c, RAW_INDEL);
    if (c->trace && !c->have_lib) fprintf(stderr, "[f2q trace] indel: every read takes k_count_indel; the deletion-variant table is built with the library\n");
    return F2Q_OK;
}

extern "C" int f2q_read_indels(f2q_ctx *c, int64_t *del_counts, int64_t *ins_counts, int64_t *del_pos, int64_t *ins_pos, int32_t n_pos, int64_t totals[4])
{
    if (!c) return F2Q_EINVAL;
    if (c->raw_mode != RAW_INDEL) return fail(c, F2Q_ESTATE, "not an indel context: call f2q_set_indel first");
    const int32_t L = c->run_h.length;
    if (n_pos != L) return fail(c, F2Q_EINVAL, "f2q_read_indels takes n_pos = L = " + std::to_string(L) + ", not " + std::to_string(n_pos));
    HIPC(c, hipSetDevice(c->device));
    const uint64_t nf = c->have_lib ? c->ix.n_features : 0, nfw = std::max<uint64_t>(nf, 1);
    std::vector<unsigned long long> h((size_t)(2 * nfw + 2 * (uint64_t)L + F2Q_INDEL_TOTALS), 0ull);
    if (c->indel.dev.del_counts) HIPC(c, hipMemcpyAsync(h.data(), c->indel.dev.del_counts, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    for (uint64_t f = 0; f < nf; f++) {
        if (del_counts) del_counts[f] = (int64_t)h[f];
        if (ins_counts) ins_counts[f] = (int64_t)h[nfw + f];
    }
    for (int32_t p = 0; p < L; p++) {
        if (del_pos) del_pos[p] = (int64_t)h[2 * nfw + p];
        if (ins_pos) ins_pos[p] = (int64_t)h[2 * nfw + L + p];
    }
    if (totals) for (int k = 0; k < F2Q_INDEL_TOTALS; k++) totals[k] = (int64_t)h[2 * nfw + 2 * L + k];
    return F2Q_OK;
}

// ---- pair libraries, each part matched alone: the ABI (include/f2q.h) -------------------------------------------------
extern "C" int f2q_set_parts(f2q_ctx *c)
{
    if (!c) return F2Q_EINVAL;
    std::string shape;
    if (!c->run_h.fixed) shape = "takes fixed windows (--st): anchored runs (--us/--ds) are not implemented";
    else if (c->n_mate1 && (c->n_mate1 != 1 || c->run_h.n_iter != 2)) shape = "on a paired context takes one window per mate, not " + std::to_string(c->n_mate1) + " + " + std::to_string(c->run_h.n_iter - c->n_mate1);
    else if (c->run_h.n_iter != 2) shape = "takes exactly two windows (--st a,b), not " + std::to_string(c->run_h.n_iter);
    if (int rc = raw_mode_enter(c, RAW_PARTS, "f2q_set_parts", shape)) return rc;
    HIPC(c, hipSetDevice(c->device));
    if (c->have_lib) if (int rc = parts_install(c, (const char *)c->ix.feat_bytes.data(), c->ix.feat_off.data(), c->ix.n_features)) return rc;   // (nothing else was touched: as if the call had not been made)
    c->parts.set.min_slots = pairset_min_slots_from_env("F2Q_PARTS_SLOTS");
    raw_road_enter(c, RAW_PARTS);
    return F2Q_OK;
}

extern "C" int f2q_parts_info(f2q_ctx *c, uint32_t *n1, uint32_t *n2)
{
    if (!c) return F2Q_EINVAL;
    if (c->raw_mode != RAW_PARTS) return fail(c, F2Q_ESTATE, "not a parts context: call f2q_set_parts first");
    if (n1) *n1 = c->parts.tab.n(0);
    if (n2) *n2 = c->parts.tab.n(1);
    return F2Q_OK;
}

extern "C" int f2q_read_parts(f2q_ctx *c, int64_t *parts_counts, int64_t *part1_reads, int64_t *part2_reads, int64_t classes[6])
{
    if (!c) return F2Q_EINVAL;
    if (c->raw_mode != RAW_PARTS) return fail(c, F2Q_ESTATE, "not a parts context: call f2q_set_parts first");
    HIPC(c, hipSetDevice(c->device));
    const PartsDev &d = c->parts.dev;
    std::vector<unsigned long long> h;
    if (d.counts) {                                              // (no library yet: nothing can have been counted)
        try { h.resize(c->parts.words); } catch (const std::bad_alloc &) { return fail(c, F2Q_ENOMEM, "no host memory to copy the part counts"); }
        HIPC(c, hipMemcpyAsync(h.data(), d.counts, c->parts.words * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    }
    unsigned long long ctr[F2Q_UMI_CTR_WORDS];
    if (int rc = pairset_read_ctr(c, c->parts.set, ctr)) return rc;
    if (h.empty()) { if (classes) for (int k = 0; k < F2Q_PARTS_CLASSES; k++) classes[k] = 0; return F2Q_OK; }
    const uint64_t nf = c->lib_h.n_features, n1 = c->parts.tab.n(0), n2 = c->parts.tab.n(1);
    if (parts_counts) for (uint64_t i = 0; i < nf; i++) parts_counts[i] = (int64_t)h[i];
    if (part1_reads) for (uint64_t i = 0; i < n1; i++) part1_reads[i] = (int64_t)h[(size_t)(d.part1 - d.counts) + i];
    if (part2_reads) for (uint64_t i = 0; i < n2; i++) part2_reads[i] = (int64_t)h[(size_t)(d.part2 - d.counts) + i];
    if (classes) for (int k = 0; k < F2Q_PARTS_CLASSES; k++) classes[k] = (int64_t)h[(size_t)(d.classes - d.counts) + k];
    return F2Q_OK;
}

// every recombinant pair with its reads, sorted by (i1, i2): the set copied and filtered on the host (no hot path)
extern "C" int f2q_parts_recombinants(f2q_ctx *c, uint64_t cap, uint64_t *n, uint32_t *part1, uint32_t *part2, uint32_t *reads)
{
    if (!c || !n) return F2Q_EINVAL;
    if (c->raw_mode != RAW_PARTS) return fail(c, F2Q_ESTATE, "not a parts context: call f2q_set_parts first");
    HIPC(c, hipSetDevice(c->device));
    const PartsDev &d = c->parts.dev;
    unsigned long long ctr[F2Q_UMI_CTR_WORDS], recombinant = 0;
    if (d.classes) HIPC(c, hipMemcpyAsync(&recombinant, d.classes + F2Q_PARTS_RECOMBINANT, sizeof recombinant, hipMemcpyDeviceToHost, c->stream));
    if (int rc = pairset_read_ctr(c, c->parts.set, ctr)) return rc;
    if (recombinant >= (1ull << 32))
        return fail(c, F2Q_EUNSUPPORTED, "f2q_parts_recombinants: 2^32 or more recombinant reads -- a pair's 32-bit count may have wrapped");
    *n = ctr[F2Q_UMI_HELD];
    if (!part1 && !part2 && !reads) return F2Q_OK;
    if (cap < *n) return fail(c, F2Q_EINVAL, "f2q_parts_recombinants: room for " + std::to_string(cap) + " pairs, the set holds " + std::to_string(*n));
    if (!*n || !d.rec.slots) return F2Q_OK;
    std::vector<unsigned long long> words; std::vector<uint32_t> cnt;
    std::vector<std::pair<unsigned long long, uint32_t>> held;
    try { words.resize(c->parts.set.n_slots); cnt.resize(c->parts.set.n_slots); held.reserve((size_t)*n); }
    catch (const std::bad_alloc &) { return fail(c, F2Q_ENOMEM, "no host memory to copy a recombinant set of " + std::to_string(c->parts.set.n_slots) + " slots"); }
    HIPC(c, hipMemcpyAsync(words.data(), d.rec.slots, c->parts.set.n_slots * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(cnt.data(), d.rec.reads, c->parts.set.n_slots * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    uint64_t occupied = 0;
    for (uint64_t i = 0; i < c->parts.set.n_slots; i++) if (words[i] != KEY_EMPTY && occupied++ < *n) held.emplace_back(words[i], cnt[i]);      // (never past the reserve)
    if (occupied != *n) return fail(c, F2Q_EHIP, "the recombinant set holds " + std::to_string(occupied) + " pairs, its counter says " + std::to_string(*n));
    std::sort(held.begin(), held.end());                         // the word is (i1 << 32) | i2
    for (size_t i = 0; i < held.size(); i++) {
        if (part1) part1[i] = (uint32_t)(held[i].first >> 32);
        if (part2) part2[i] = (uint32_t)held[i].first;
        if (reads) reads[i] = held[i].second;
    }
    return F2Q_OK;
}

// F2Q_TRACE_SYNC=1: name every step of the Extract+Count path on stderr and wait for it (fault localisation only)
#define EC_POINT(c, what) do { if ((c)->trace_sync) { (void)hipStreamSynchronize((c)->stream); fprintf(stderr, "[f2q sync] %s done\n", what); fflush(stderr); } } while (0)

// ---- Extract+Count table management -----------------------------------------------------------
// the two sides of the Extract+Count tables grow independently: the single-word table (k64_*: one slot per plain ACGT
// key of <= 29 bases) and the byte-string table (slots, entry arrays, arena); the four counters outlive both
static int ec_alloc64(f2q_ctx *c, EcDev &e, std::vector<void *> &owner, uint64_t max_keys64)
{
    // load factor <= 0.75: smaller tables are cheaper to clear and stay in the Infinity Cache longer
    uint64_t slots64 = 1024;
    while (3 * slots64 < 4 * max_keys64) slots64 <<= 1;
    if (slots64 > (1ull << 32)) return fail(c, F2Q_ENOMEM, "Extract+Count table would exceed 2^32 slots");
    int rc;
    if ((rc = dev_alloc(c, slots64, &e.k64_slots, owner, 0xFF))) return rc;
    if ((rc = dev_alloc(c, slots64, &e.k64_count, owner, 0))) return rc;
    if ((rc = dev_alloc(c, slots64, &e.k64_first, owner, 0xFF))) return rc;
    e.k64_mask = (uint32_t)(slots64 - 1);
    e.k64_room = (uint32_t)std::min<uint64_t>(3 * slots64 / 4, 0xFFFFFFFEull);   // keys the table takes before it must grow
    return F2Q_OK;
}
static int ec_allocB(f2q_ctx *c, EcDev &e, std::vector<void *> &owner, uint64_t max_entries, uint64_t arena_words)
{
    uint64_t slots = 1024;
    while (3 * slots < 4 * max_entries) slots <<= 1;
    if (slots > (1ull << 32)) return fail(c, F2Q_ENOMEM, "Extract+Count table would exceed 2^32 slots");
    int rc;
    if ((rc = dev_alloc(c, slots, &e.slots, owner, 0))) return rc;
    if ((rc = dev_alloc(c, max_entries, &e.ent_off, owner))) return rc;
    if ((rc = dev_alloc(c, max_entries, &e.ent_len, owner))) return rc;
    if ((rc = dev_alloc(c, max_entries, &e.ent_count, owner, 0))) return rc;
    if ((rc = dev_alloc(c, max_entries, &e.ent_first, owner, 0xFF))) return rc;
    if ((rc = dev_alloc(c, arena_words, &e.arena, owner))) return rc;
    e.mask = (uint32_t)(slots - 1); e.max_entries = (uint32_t)std::min<uint64_t>(max_entries, 0xFFFFFFFEull);
    e.arena_words = arena_words;
    return F2Q_OK;
}

// make room for `keys64` more keys in the single-word table and `reads` more entries of at most `key_bytes` bytes in
// the byte-string table
// known: the counters as the caller has just read them (nothing has run since), else they are fetched
static int ec_reserve(f2q_ctx *c, uint64_t keys64, uint64_t reads, uint64_t key_bytes, const unsigned long long *known = nullptr)
{
    unsigned long long ctr[4] = {0, 0, 0, 0};
    if (known) memcpy(ctr, known, sizeof ctr);
    else if (c->ec.ctr) {
        HIPC(c, hipMemcpyAsync(ctr, c->ec.ctr, sizeof ctr, hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipStreamSynchronize(c->stream));
        if (ctr[2]) return fail(c, F2Q_ENOMEM, "Extract+Count table overflow (internal sizing error, code " + std::to_string(ctr[2]) + ")");
    }
    // the byte-string table is limited by its entry arrays and its arena, the single-word table by its load factor (<= 3/4)
    const uint64_t need_b = ctr[0] + reads + 16, need_r = ctr[3] + keys64 + 16, need_w = ctr[1] + (key_bytes + 3) / 4 + reads + 16;
    const bool grow64 = !c->ec.k64_slots || need_r > c->ec.k64_room;
    const bool growB = !c->ec.slots || need_b > c->ec.max_entries || need_w > c->ec.arena_words;
    if (!grow64 && !growB) return F2Q_OK;
    const double rs0 = now_ms();
    c->ec_gen++;                                                 // the tables move: per-key arrays of an earlier assign are stale
    // nothing may still be counting into the tables that are about to move
    if (c->aux_busy) { HIPC(c, hipStreamSynchronize(c->aux_stream)); c->aux_busy = false; }
    if (c->ec.ctr) {                                             // the exact counters: they say how much is carried over
        HIPC(c, hipMemcpyAsync(ctr, c->ec.ctr, sizeof ctr, hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipStreamSynchronize(c->stream));
        if (ctr[2]) return fail(c, F2Q_ENOMEM, "Extract+Count table overflow (internal sizing error, code " + std::to_string(ctr[2]) + ")");
    }
    int rc;
    if (!c->ec.ctr && (rc = dev_alloc(c, (size_t)F2Q_CTR_WORDS, &c->ec.ctr, c->ec_allocs_ctr, 0))) return rc;
    if ((c->ec.k64_slots && grow64 && ctr[3]) || (c->ec.slots && growB && ctr[0])) {
        c->n_rehash++;
        if (c->trace && c->n_rehash <= 6)
            fprintf(stderr, "[f2q trace] Extract+Count tables grow (%s%s): keys %llu/%llu, entries needed %llu of %u, single-word keys needed %llu of %u, arena words needed %llu of %llu\n",
                    grow64 ? "single-word " : "", growB ? "byte-string" : "", ctr[0], ctr[3], (unsigned long long)need_b, c->ec.max_entries,
                    (unsigned long long)need_r, c->ec.k64_room, (unsigned long long)need_w, c->ec.arena_words);
    }
    // growth doubles the room of the keys already there (amortised rehash), not the head room of one launch
    if (grow64) {
        const uint64_t nr = std::max<uint64_t>(need_r + std::max<uint64_t>(ctr[3], keys64 / 4), 1u << 16);
        EcDev fresh = c->ec; std::vector<void *> owner;
        if ((rc = ec_alloc64(c, fresh, owner, nr))) { free_all(c, owner); return rc; }
        if (c->ec.k64_slots && ctr[3]) {
            hipLaunchKernelGGL(k_ec64_rehash, dim3((unsigned)(((uint64_t)c->ec.k64_mask + 256) / 256)), dim3(256), 0, c->stream, c->ec, fresh);
            HIPC(c, hipGetLastError());
            EC_POINT(c, "reserve: k_ec64_rehash");
            if (c->hot_valid) {                                  // the hot keys' slots moved with the table
                hipLaunchKernelGGL(k_ec_hot_relink, dim3(F2Q_HOT_SLOTS / 256), dim3(256), 0, c->stream, fresh, c->hot);
                HIPC(c, hipGetLastError());
                EC_POINT(c, "reserve: k_ec_hot_relink");
            }
        }
        free_all(c, c->ec_allocs64);                             // (waits for the stream)
        c->ec_allocs64 = owner;
        c->ec.k64_slots = fresh.k64_slots; c->ec.k64_count = fresh.k64_count; c->ec.k64_first = fresh.k64_first;
        c->ec.k64_mask = fresh.k64_mask; c->ec.k64_room = fresh.k64_room;
    }
    if (growB) {
        const uint64_t nb = need_b > c->ec.max_entries || !c->ec.slots ? std::max<uint64_t>(need_b + std::max<uint64_t>(ctr[0], reads / 4), 1u << 12)
                                                                        : (uint64_t)c->ec.max_entries;
        const uint64_t nw = need_w > c->ec.arena_words || !c->ec.slots ? std::max<uint64_t>(need_w + std::max<uint64_t>(ctr[1], key_bytes / 16), 1u << 14)
                                                                       : c->ec.arena_words;
        EcDev fresh = c->ec; std::vector<void *> owner;
        if ((rc = ec_allocB(c, fresh, owner, nb, nw))) { free_all(c, owner); return rc; }
        if (c->ec.slots && ctr[0]) {
            HIPC(c, hipMemcpyAsync(fresh.arena, c->ec.arena, ctr[1] * 4, hipMemcpyDeviceToDevice, c->stream));
            HIPC(c, hipMemcpyAsync(fresh.ent_off, c->ec.ent_off, ctr[0] * 8, hipMemcpyDeviceToDevice, c->stream));
            HIPC(c, hipMemcpyAsync(fresh.ent_len, c->ec.ent_len, ctr[0] * 4, hipMemcpyDeviceToDevice, c->stream));
            HIPC(c, hipMemcpyAsync(fresh.ent_count, c->ec.ent_count, ctr[0] * 8, hipMemcpyDeviceToDevice, c->stream));
            HIPC(c, hipMemcpyAsync(fresh.ent_first, c->ec.ent_first, ctr[0] * 8, hipMemcpyDeviceToDevice, c->stream));
            hipLaunchKernelGGL(k_ec_rehash, dim3((unsigned)((ctr[0] + 255) / 256)), dim3(256), 0, c->stream, c->ec, ctr[0], fresh);
            HIPC(c, hipGetLastError());
            EC_POINT(c, "reserve: k_ec_rehash");
        }
        free_all(c, c->ec_allocs);
        c->ec_allocs = owner;
        c->ec.slots = fresh.slots; c->ec.mask = fresh.mask; c->ec.max_entries = fresh.max_entries;
        c->ec.ent_off = fresh.ent_off; c->ec.ent_len = fresh.ent_len; c->ec.ent_count = fresh.ent_count; c->ec.ent_first = fresh.ent_first;
        c->ec.arena = fresh.arena; c->ec.arena_words = fresh.arena_words;
    }
    c->tr_reserve += now_ms() - rs0;
    return F2Q_OK;
}

// ---- launching ----------------------------------------------------------------------------------
// a device buffer of at least `want` elements; it only grows (the old contents are not kept)
template <class T>
static int grow_buf(f2q_ctx *c, T **buf, size_t &have, size_t want, bool zero)
{
    if (want <= have) return F2Q_OK;
    HIPC(c, hipStreamSynchronize(c->stream));
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr; have = 0;
    HIPC(c, hipMalloc((void **)buf, want * sizeof(T)));
    if (zero) HIPC(c, hipMemsetAsync(*buf, 0, want * sizeof(T), c->stream));
    have = want;
    return F2Q_OK;
}
// the per-workgroup rows of a launch that reduces through k_reduce_slabs: `rows` histogram rows of n_features counts and
// `stat_rows` rows of 8 stats; acc points at them
static int slab_rows(f2q_ctx *c, size_t rows, size_t stat_rows, Accum &acc)
{
    int rc;
    if ((rc = grow_buf(c, &c->slab_d, c->slab_n, std::max<size_t>(rows * c->lib_h.n_features, 1), false))) return rc;
    if ((rc = grow_buf(c, &c->stat_slab_d, c->stat_slab_n, stat_rows * 8, false))) return rc;
    acc.slab = c->slab_d; acc.stat_slab = c->stat_slab_d;
    return F2Q_OK;
}
// k_reduce_slabs: the launch's `rows` histogram rows and `stat_rows` stats rows into the accumulators.  Where a reset
// left the clear pending the reduce stores and the clear is no work at all; the caller has made sure (acc_ready) that no
// kernel queued since that reset has added to the accumulators
static int reduce_slabs(f2q_ctx *c, const Accum &acc, uint32_t rows, uint32_t stat_rows, uint32_t &launches)
{
    const uint32_t nf = c->lib_h.n_features;
    const uint32_t store = c->acc_pending ? 1u : 0u;
    // a workgroup per F2Q_RED_FEATS features, and one more for the five counters
    hipLaunchKernelGGL(k_reduce_slabs, dim3((nf + F2Q_RED_FEATS - 1) / F2Q_RED_FEATS + 1u), dim3(256), 0, c->stream,
                       c->slab_d, rows, nf, acc.counts, acc.carry, c->stat_slab_d, stat_rows, acc.stats, store);
    HIPC(c, hipGetLastError());
    c->acc_pending = false;                          // (only now: a launch that failed has cleared nothing)
    launches++;
    return F2Q_OK;
}
// hipFuncAttributeMaxDynamicSharedMemorySize of a kernel: set once per device and kernel, again only for a larger size
static int dyn_lds(f2q_ctx *c, const void *kern, size_t shmem)
{
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, size_t> set;
    std::lock_guard<std::mutex> lock(mu);
    size_t &have = set[{c->device, kern}];
    if (shmem <= have) return F2Q_OK;
    HIPC(c, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    have = shmem;
    return F2Q_OK;
}
static bool same_q(const RunDev &r) { return r.thr_up == r.thr && r.thr_down == r.thr; }

// calls f(NW, KB, SQ) with the std::integral_constant arguments of an anchored geometry: nw 3 or 5, kb 0, 1 or 3,
// SQ = sameq.  WIDE: nw 10 (reads of 161 .. 320 bases) has one general instantiation, <10, 3, false> (any --msu/--msd
// <= 7, any --qsu/--qsd); only k_count_anchor and k_count_anchor_pairs have it.
template <int N> using int_c = std::integral_constant<int, N>;
template <bool WIDE = false, class F>
static void anchored_geom(int nw, int kb, bool sameq, F &&f)
{
    if constexpr (WIDE) {
        if (nw == 10) return f(int_c<10>(), int_c<3>(), std::false_type());
    }
    auto by_kb = [&](auto NW) {
        auto by_sq = [&](auto KB) { if (sameq) f(NW, KB, std::true_type()); else f(NW, KB, std::false_type()); };
        if (kb == 0) by_sq(int_c<0>()); else if (kb == 1) by_sq(int_c<1>()); else by_sq(int_c<3>());
    };
    if (nw == 3) by_kb(int_c<3>()); else by_kb(int_c<5>());
}

// the specialisation of the fixed-window kernels for a window: spec52 (5 quality rows, 2 base rows), a20 (spec52 with
// a 20-base window at a 16-aligned start) or the run-time geometry
enum FixedVariant { FV_GENERIC, FV_SPEC52, FV_A20 };
static FixedVariant fixed_variant(const f2q_ctx *c, const FixedGeom &g)
{
    if (c->force_generic || g.nq != 5 || g.nb != 2 || c->run_h.thr < 33) return FV_GENERIC;
    return g.L == 20 && (g.st & 15) == 0 ? FV_A20 : FV_SPEC52;
}

// the kernel family that counts a view's packed tiles (F2Q_PATH_*; pb.n_tiles > 0)
static uint32_t choose_path(const f2q_ctx *c, const PackedBlock &pb)
{
    const bool ecm = c->prm.mode == 1;
    // the library in LDS: uniform 14..21-base library, --m <= 1
    const bool lt = c->lib_h.n_features <= F2Q_HIST_MAX && !c->no_lt && c->lib_h.lt.ok && c->run_h.miss <= 1 && pb.len != nullptr;
    if (pb.planar_nw) {
        if (c->plan.multi_pair) return F2Q_PATH_PAIRS;           // several --us/--ds pairs on the planes
        if (ecm) return F2Q_PATH_EXTRACT;
        return lt && same_q(c->run_h) && pb.planar_nw != 10 ? F2Q_PATH_ANCHOR_LDS : F2Q_PATH_ANCHOR;
    }
    if (ecm) return F2Q_PATH_EXTRACT;
    if (c->plan.multi) {
        // several windows per read, every feature with one part per window: the joined keys on the library-in-LDS
        // kernel (the tiles hold the windows back to back: one window of n_iter * length bases)
        const uint32_t mw_total = (uint32_t)(c->run_h.n_iter * c->run_h.length);
        const bool mw_lt = lt && c->lib_h.lt.len == mw_total && (mw_total + 3) / 4 <= pb.wq && (mw_total + 15) / 16 <= pb.wb;
        return mw_lt ? F2Q_PATH_MULTI_LDS : F2Q_PATH_MULTI;
    }
    const uint32_t len = (uint32_t)c->run_h.length;
    const bool v2 = !c->force_v1 && c->lib_h.pk.len == len && len > 0 && c->lib_h.n_irregular == 0;
    const FixedGeom g = fixed_geom(c->run_h);
    // the tiles hold every row under the window
    const bool rows = v2 && c->run_h.miss <= 1 && (uint32_t)(g.qw0 + g.nq) <= pb.wq && (uint32_t)(g.bw0 + g.nb) <= pb.wb && pb.len != nullptr;
    const bool use_lt = rows && lt && c->lib_h.lt.len == len;
    // a library beyond one workgroup's LDS, dealt into partitions (or F2Q_PT_PARTS set: that path whatever the size)
    if (rows && !c->no_pt && c->lib_h.pt.ok && c->lib_h.pt.len == len &&
        (c->ix.pt_force_parts > 0 || (!use_lt && (uint64_t)pb.n_tiles * F2Q_TILE >= c->pt_min_reads)))
        return F2Q_PATH_FIXED_PART;
    if (use_lt) return F2Q_PATH_FIXED_LDS;
    return v2 ? F2Q_PATH_FIXED_PACKED : F2Q_PATH_FIXED_V1;
}

// several --us/--ds pairs on the planes
static int launch_pairs(f2q_ctx *c, const PackedBlock &pb, Accum &acc, uint32_t &launches)
{
    const bool lds = c->prm.mode == 0 && c->lib_h.n_features <= F2Q_HIST_MAX;
    uint32_t grid = std::min<uint32_t>(pb.n_tiles, (uint32_t)c->n_cu * 8u);                // (four workgroups of 256 threads are resident per CU at 128 VGPRs: two rounds)
    if (c->lt_max_wgs) grid = std::min<uint32_t>(grid, c->lt_max_wgs);
    const size_t shmem = lds ? std::max<size_t>(4, (((size_t)c->lib_h.n_features + 1) / 2) * 4) : 4;
    anchored_geom<true>(pb.planar_nw, c->plan.kb, same_q(c->run_h), [&](auto NW, auto KB, auto SQ) {
        auto kern = lds ? k_count_anchor_pairs<NW, KB, SQ, true> : k_count_anchor_pairs<NW, KB, SQ, false>;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(F2Q_AN_THREADS), shmem, c->stream, c->run_d, c->lib_d, c->ec, pb, acc, c->reads_seen);
    });
    HIPC(c, hipGetLastError());
    launches++;
    return F2Q_OK;
}

// packed anchored path: Counter mode (per-workgroup histogram in LDS up to F2Q_HIST_MAX features) or Extract+Count
static int launch_anchor(f2q_ctx *c, const PackedBlock &pb, Accum &acc, uint32_t &launches)
{
    const bool ecm = c->prm.mode == 1;
    const uint32_t nf = c->lib_h.n_features;
    const bool lds = !ecm && nf <= F2Q_HIST_MAX;
    const uint32_t grid = std::min<uint32_t>(pb.n_tiles, (uint32_t)c->n_cu * 4u);
    const size_t shmem = (size_t)F2Q_AN_WAVES * F2Q_AN_QCAP * 12 + (lds ? (size_t)nf * 4 : 0);
    int rc;
    if (lds && (rc = slab_rows(c, grid, grid, acc))) return rc;
    anchored_geom<true>(pb.planar_nw, c->plan.kb, same_q(c->run_h), [&](auto NW, auto KB, auto SQ) {
        auto kern = ecm ? k_count_anchor<NW, KB, true, false, SQ> : lds ? k_count_anchor<NW, KB, false, true, SQ> : k_count_anchor<NW, KB, false, false, SQ>;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(F2Q_AN_THREADS), shmem, c->stream, c->run_d, c->lib_d, c->ec, pb, acc, c->reads_seen);
    });
    HIPC(c, hipGetLastError());
    launches++;
    return lds && nf ? reduce_slabs(c, acc, grid, grid, launches) : F2Q_OK;
}

// anchored tiles with the library in LDS (Counter mode, default --qsu/--qsd)
static int launch_anchor_lds(f2q_ctx *c, const PackedBlock &pb, Accum &acc, uint32_t &launches)
{
    const uint32_t groups = (pb.n_tiles + F2Q_ALT_GROUPS - 1) / F2Q_ALT_GROUPS;
    uint32_t grid = std::min<uint32_t>(groups, (uint32_t)c->n_cu);
    if (c->lt_max_wgs) grid = std::min<uint32_t>(grid, c->lt_max_wgs);
    const bool near = c->run_h.miss > 0;
    const size_t shmem = ((near ? 2u : 1u) * (size_t)F2Q_LT_SLOTS + F2Q_LT_BUCKETS) * 4;
    int rc = slab_rows(c, grid, grid, acc);
    if (rc) return rc;
    // (this path is taken with sameq only: the kernel has no SAMEQ = false instance)
    anchored_geom(pb.planar_nw, c->plan.kb, true, [&](auto NW, auto KB, auto) {
        auto kern = near ? k_count_anchor_lt<NW, KB, true, true> : k_count_anchor_lt<NW, KB, true, false>;
        if ((rc = dyn_lds(c, (const void *)kern, shmem))) return;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(F2Q_ALT_THREADS), shmem, c->stream, c->run_d, c->lib_d, pb, acc);
    });
    if (rc) return rc;
    HIPC(c, hipGetLastError());
    launches++;
    return reduce_slabs(c, acc, grid, grid, launches);
}

// Extract+Count on fixed-window tiles, one step of the block (where the hot-key kernels are not taken: ec_hot_path)
static int launch_extract_fixed(f2q_ctx *c, const PackedBlock &pb, Accum &acc, uint32_t &launches)
{
    const uint32_t wgs = (pb.n_tiles + F2Q_V2_WAVES - 1) / F2Q_V2_WAVES;
    const uint32_t grid = std::min<uint32_t>(wgs, (uint32_t)c->n_cu * 4u);
    hipLaunchKernelGGL(k_extract_fixed4, dim3(grid), dim3(F2Q_V2_THREADS), 0, c->stream, c->run_d, c->ec, pb, acc, c->reads_seen);
    HIPC(c, hipGetLastError());
    launches++;
    return F2Q_OK;
}

// several windows per read (--st a,b,...): k-part keys against the k-part features
static int launch_multi(f2q_ctx *c, const PackedBlock &pb, Accum &acc, uint32_t &launches)
{
    const uint32_t nf = c->lib_h.n_features;
    const bool lds = nf <= F2Q_HIST_MAX;
    const uint32_t wgs = (pb.n_tiles + F2Q_V2_WAVES - 1) / F2Q_V2_WAVES;
    uint32_t grid = std::min<uint32_t>(wgs, (uint32_t)c->n_cu * 2u);
    if (c->lt_max_wgs) grid = std::min<uint32_t>(grid, c->lt_max_wgs);
    const size_t shmem = (size_t)F2Q_V2_WAVES * F2Q_V2_QCAP * 12 + (lds ? (size_t)nf * 4 : 0);
    int rc = slab_rows(c, lds ? grid : 0u, grid, acc);
    if (rc) return rc;
    auto kern = lds ? k_count_multi4<true> : k_count_multi4<false>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(F2Q_V2_THREADS), shmem, c->stream, c->run_d, c->lib_d, pb, acc, c->plan.need);
    HIPC(c, hipGetLastError());
    launches++;
    return reduce_slabs(c, acc, lds ? grid : 0u, grid, launches);
}

// fixed-offset Counter mode on a partitioned library: the block's tiles in chunks, each scattered and then counted
static int launch_part(f2q_ctx *c, const PackedBlock &pb, Accum &acc, uint32_t &launches)
{
    const PtDesc &pt = c->lib_h.pt;
    const uint32_t P = pt.n_parts, nf = c->lib_h.n_features;
    const int pw = P <= 8 ? 16 : P <= 16 ? 8 : 4;                    // scatter waves per workgroup: n_parts KiB of rings each
    // rounds of equal size, none above pt_chunk_reads (the scratch memory of a round is 8 bytes x partitions x its reads)
    // ... and that memory is kept to 16 GiB (a stream must be able to take every entry of its workgroup)
    const uint64_t chunk_reads = std::min<uint64_t>(c->pt_chunk_reads, ((uint64_t)16 << 30) / (8ull * P));
    const uint32_t max_tiles = (uint32_t)std::max<uint64_t>(chunk_reads / F2Q_TILE, 1);
    const uint32_t n_rounds = std::max<uint32_t>(1u, (pb.n_tiles + max_tiles - 1) / max_tiles);
    const uint32_t chunk_tiles = std::max<uint32_t>(1u, (pb.n_tiles + n_rounds - 1) / n_rounds);
    uint32_t grid1 = std::min<uint32_t>((uint32_t)c->n_cu, (chunk_tiles + pw - 1) / pw);
    if (c->lt_max_wgs) grid1 = std::min<uint32_t>(grid1, c->lt_max_wgs);                    // (before the stream capacity is derived from it)
    const uint32_t tiles_per_wg = (chunk_tiles + grid1 - 1) / grid1 + (uint32_t)pw;          // (waves take tiles round robin)
    // entries per stream: what a workgroup can produce, in whole steps of the count pass, plus 11 x 256 bytes: the streams
    // grow at the same pace, and at a power-of-two distance their write positions would share memory channels
    const uint32_t cap = ((tiles_per_wg * F2Q_TILE + F2Q_PC_STEP - 1) / F2Q_PC_STEP) * F2Q_PC_STEP + F2Q_PC_STEP + 352u;
    const uint32_t K = std::max<uint32_t>(1u, (uint32_t)c->n_cu / P), grid2 = K * P, cw = F2Q_PC_THREADS / 64;
    if ((grid1 + K - 1) / K > 64) return fail(c, F2Q_EUNSUPPORTED, "partitioned path: more than 64 streams per counting workgroup");
    const uint32_t n_slots1 = 2u << pt.bb1, rows = grid1 + grid2;
    int rc;
    if ((rc = grow_buf(c, &c->pt_s.streams, c->pt_streams_n, (size_t)grid1 * P * cap, false))) return rc;
    if ((rc = grow_buf(c, &c->pt_s.cnt, c->pt_cnt_n, (size_t)grid1 * P, false))) return rc;
    if ((rc = grow_buf(c, &c->pt_slab0_d, c->pt_slab0_n, (size_t)grid2 * std::max<uint32_t>(pt.max_part, 1u), true))) return rc;
    if ((rc = grow_buf(c, &c->pt_slab1_d, c->pt_slab1_n, (size_t)n_slots1, true))) return rc;
    if ((rc = grow_buf(c, &c->pt_stat_d, c->pt_stat_n, (size_t)rows * 8, true))) return rc;     // rows accumulate; k_part_reduce clears them
    PartScratch ps = c->pt_s;
    ps.cap = cap; ps.n_wg1 = grid1;
    Accum a1 = acc, a2 = acc;
    a1.stat_slab = c->pt_stat_d; a2.stat_slab = a1.stat_slab + (size_t)grid1 * 8;
    const FixedVariant fv = fixed_variant(c, fixed_geom(c->run_h));
    const bool near = c->run_h.miss > 0;
    const size_t shmem1 = (size_t)pw * P * F2Q_PS_RING * 8 + (size_t)(pw + 1) * P * 4;
    const size_t shmem2 = ((size_t)F2Q_LT_SLOTS + F2Q_LT_BUCKETS) * 4 + (near ? (size_t)cw * (F2Q_PC_RING * 8 + F2Q_PC_VIA * 4) : 0);
    auto kern2 = near ? k_part_count<true> : k_part_count<false>;
    if ((rc = dyn_lds(c, (const void *)kern2, shmem2))) return rc;
    for (uint32_t t0 = 0; t0 < pb.n_tiles; t0 += chunk_tiles) {
        const uint32_t t1 = std::min<uint32_t>(pb.n_tiles, t0 + chunk_tiles);
        auto scatter = [&](auto PW) {
            auto k1 = fv == FV_A20 ? k_part_scatter<5, 2, true, PW> : fv == FV_SPEC52 ? k_part_scatter<5, 2, false, PW> : k_part_scatter<0, 0, false, PW>;
            if ((rc = dyn_lds(c, (const void *)k1, shmem1))) return;
            hipLaunchKernelGGL(k1, dim3(grid1), dim3(64 * PW), shmem1, c->stream, c->run_d, c->lib_d, pb, a1, ps, t0, t1);
        };
        if (pw == 16) scatter(int_c<16>()); else if (pw == 8) scatter(int_c<8>()); else scatter(int_c<4>());
        if (rc) return rc;
        HIPC(c, hipGetLastError());
        hipLaunchKernelGGL(kern2, dim3(grid2), dim3(64 * cw), shmem2, c->stream, c->run_d, c->lib_d, a2, ps, c->pt_slab0_d, c->pt_slab1_d);
        HIPC(c, hipGetLastError());
        launches += 2;
    }
    hipLaunchKernelGGL(k_part_reduce, dim3(std::max<uint32_t>(1u, (nf + 63) / 64)), dim3(256), 0, c->stream, c->lib_d, c->pt_slab0_d, K,
                       near ? c->pt_slab1_d : (uint32_t *)nullptr, acc.counts, c->pt_stat_d, rows, acc.stats);
    HIPC(c, hipGetLastError());
    launches++;
    return F2Q_OK;
}

// the library in LDS (k_count_fixed4_lds): one fixed window (tiles that hold every row under it), or, mw, several
// windows joined into one (Phred rule per part)
template <bool MW>
static auto fixed_lds_kernel(bool near, FixedVariant fv)
{
    if (near) return fv == FV_A20 ? k_count_fixed4_lds<5, 2, true, true, MW> : fv == FV_SPEC52 ? k_count_fixed4_lds<5, 2, true, false, MW> : k_count_fixed4_lds<0, 0, true, false, MW>;
    return fv == FV_A20 ? k_count_fixed4_lds<5, 2, false, true, MW> : fv == FV_SPEC52 ? k_count_fixed4_lds<5, 2, false, false, MW> : k_count_fixed4_lds<0, 0, false, false, MW>;
}
static int launch_fixed_lds(f2q_ctx *c, const PackedBlock &pb, Accum &acc, uint32_t &launches, bool mw)
{
    const uint32_t wgs = (pb.n_tiles + F2Q_LT_WAVES - 1) / F2Q_LT_WAVES;
    const uint32_t grid = std::min<uint32_t>(wgs, c->lt_max_wgs ? std::min<uint32_t>(c->lt_max_wgs, (uint32_t)c->n_cu) : (uint32_t)c->n_cu);
    const bool near = c->run_h.miss > 0;
    const size_t shmem = ((near ? 2u : 1u) * (size_t)F2Q_LT_SLOTS + F2Q_LT_BUCKETS) * 4;
    const FixedVariant fv = fixed_variant(c, mw ? fixed_geom_at(0, c->run_h.n_iter * c->run_h.length, c->run_h.thr) : fixed_geom(c->run_h));
    auto kern = mw ? fixed_lds_kernel<true>(near, fv) : fixed_lds_kernel<false>(near, fv);
    int rc = slab_rows(c, grid, grid, acc);
    if (rc) return rc;
    if ((rc = dyn_lds(c, (const void *)kern, shmem))) return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(F2Q_LT_THREADS), shmem, c->stream, c->run_d, c->lib_d, pb, acc);
    HIPC(c, hipGetLastError());
    launches++;
    return reduce_slabs(c, acc, grid, grid, launches);
}

// packed tables in L2 (k_count_fixed4): histogram in LDS, or, beyond F2Q_HIST_MAX features, a feature index per read slot
// binned by k_hist_ranges
static int launch_fixed_packed(f2q_ctx *c, const PackedBlock &pb, Accum &acc, uint32_t &launches)
{
    const uint32_t nf = c->lib_h.n_features;
    const bool lds = nf <= F2Q_HIST_MAX;
    const uint32_t wgs = (pb.n_tiles + F2Q_V2_WAVES - 1) / F2Q_V2_WAVES;
    uint32_t grid = std::min<uint32_t>(wgs, (uint32_t)c->n_cu * 2u);
    if (c->lt_max_wgs) grid = std::min<uint32_t>(grid, c->lt_max_wgs);
    const size_t shmem = (size_t)F2Q_V2_WAVES * F2Q_V2_QCAP * 12 + (lds ? (size_t)nf * 4 : (size_t)F2Q_V2_WAVES * F2Q_V2_QCAP * 4);
    const bool spec52 = fixed_variant(c, fixed_geom(c->run_h)) != FV_GENERIC;      // (no a20 instance: spec52 serves it)
    auto kern = lds ? (spec52 ? k_count_fixed4<true, 5, 2> : k_count_fixed4<true, 0, 0>)
                    : (spec52 ? k_count_fixed4<false, 5, 2> : k_count_fixed4<false, 0, 0>);
    const uint32_t n_ranges = lds ? 1u : (nf + F2Q_HIST_RANGE - 1) / F2Q_HIST_RANGE;
    const uint32_t n_parts = lds ? grid : std::max<uint32_t>(1u, (uint32_t)c->n_cu / n_ranges);
    // slab rows: one per counting workgroup (LDS histogram) or one per part of k_hist_ranges; stats rows per workgroup
    int rc = slab_rows(c, n_parts, grid, acc);
    if (rc) return rc;
    if (!lds) {
        if ((rc = grow_buf(c, &c->hit_buf_d, c->hit_buf_n, pb.n_slots, false))) return rc;
        acc.hit_buf = c->hit_buf_d;                          // (the kernel writes every slot: no clearing)
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(F2Q_V2_THREADS), shmem, c->stream, c->run_d, c->lib_d, pb, acc);
    HIPC(c, hipGetLastError());
    launches++;
    if (!lds && nf) {
        if ((rc = dyn_lds(c, (const void *)k_hist_ranges, (size_t)F2Q_HIST_RANGE * 4))) return rc;
        hipLaunchKernelGGL(k_hist_ranges, dim3(n_ranges * n_parts), dim3(1024), (size_t)F2Q_HIST_RANGE * 4, c->stream,
                           c->hit_buf_d, (uint64_t)pb.n_slots, nf, n_parts, c->slab_d);
        HIPC(c, hipGetLastError());
        launches++;
    }
    return nf ? reduce_slabs(c, acc, n_parts, grid, launches) : F2Q_OK;
}

// one read per lane, wide tables: libraries the packed tables do not serve, or F2Q_FORCE_V1=1
static int launch_fixed_v1(f2q_ctx *c, const PackedBlock &pb, Accum &acc, uint32_t &launches)
{
    const uint32_t grid = std::min<uint32_t>(pb.n_tiles, (uint32_t)c->n_cu * 8u);
    if (c->lib_h.n_features <= F2Q_HIST_MAX) {
        const size_t shmem = std::max<size_t>(4, (size_t)c->lib_h.n_features * 4);
        hipLaunchKernelGGL(k_count_fixed<true>, dim3(grid), dim3(F2Q_TILE), shmem, c->stream, c->run_d, c->lib_d, pb, acc);
    } else {
        hipLaunchKernelGGL(k_count_fixed<false>, dim3(grid), dim3(F2Q_TILE), 0, c->stream, c->run_d, c->lib_d, pb, acc);
    }
    HIPC(c, hipGetLastError());
    launches++;
    return F2Q_OK;
}

// ---- pair sets: the (feature, UMI) set of a UMI context, the recombinant set of a parts context -----------------------
// The set before a launch over n records: afterwards it is at most half full even if every record brings a new pair, so
// the counting kernel always finds room.  The pairs held are read from the device only when the bound kept on the host
// says the set might be too small; a set that is grows to hold twice what it must (amortised rehash).  The new set is
// allocated before the old one is given back: a failed allocation leaves the context as it was.  With reads kept
// (f2q_set_umi_reads; always for recombinants) reads[] comes and goes with slots[]: allocated zeroed next to it, filled by
// the rehash.
static int pairset_reserve(f2q_ctx *c, PairSet &s, uint64_t n)
{
    int rc;
    UmiDev &u = *s.dev;
    if (u.slots && 2 * (s.held_ub + n) <= s.n_slots) { s.held_ub += n; return F2Q_OK; }
    unsigned long long ctr[F2Q_UMI_CTR_WORDS] = {0, 0, 0, 0};
    if (u.slots) {
        if ((rc = pairset_read_ctr(c, s, ctr))) return rc;
        if (2 * (ctr[F2Q_UMI_HELD] + n) <= s.n_slots) { s.held_ub = ctr[F2Q_UMI_HELD] + n; return F2Q_OK; }
    }
    const uint64_t held = ctr[F2Q_UMI_HELD];
    uint64_t slots = std::max<uint64_t>(s.min_slots, 2);
    while (slots < 2 * (held + n) || slots < 4 * held) slots <<= 1;
    if (slots > (1ull << 32)) return fail(c, F2Q_ENOMEM, std::string("the ") + s.name + " set would exceed 2^32 slots");
    UmiDev fresh = u; std::vector<void *> owner;
    if ((rc = dev_alloc(c, (size_t)slots, &fresh.slots, owner, 0xFF)) ||
        (s.keep_reads && (rc = dev_alloc(c, (size_t)slots, &fresh.reads, owner, 0)))) {
        free_all(c, owner);
        return fail(c, F2Q_ENOMEM, std::string("no device memory for a ") + s.name + " set of " + std::to_string(slots) + " slots: " + c->err);
    }
    fresh.mask = (uint32_t)(slots - 1);
    if (u.slots && held) {
        if (u.reads) hipLaunchKernelGGL(k_umi_rehash<true>, dim3((unsigned)((s.n_slots + 255) / 256)), dim3(256), 0, c->stream, u, fresh);
        else hipLaunchKernelGGL(k_umi_rehash<false>, dim3((unsigned)((s.n_slots + 255) / 256)), dim3(256), 0, c->stream, u, fresh);
        HIPC(c, hipGetLastError());
        s.rehashes++;
        if (c->trace) fprintf(stderr, "[f2q trace] %s set rehash %llu: %llu pairs, %llu -> %llu slots\n", s.name, (unsigned long long)s.rehashes,
                              (unsigned long long)held, (unsigned long long)s.n_slots, (unsigned long long)slots);
    }
    free_all(c, s.set_allocs);                                   // (waits for the stream)
    s.set_allocs = owner;
    u.slots = fresh.slots; u.reads = fresh.reads; u.mask = fresh.mask; s.n_slots = slots;
    s.held_ub = held + n;
    return F2Q_OK;
}

// ---- distinct UMIs per feature -------------------------------------------------------------------------------------
// umis[] and the set's counters, with the first launch after f2q_set_umi or a new library
static int umi_counters(f2q_ctx *c)
{
    if (c->umi.dev.umis) return F2Q_OK;
    UmiDev u = c->umi.dev; std::vector<void *> owner;
    if (dev_alloc(c, (size_t)std::max<uint64_t>(c->lib_h.n_features, 1), &u.umis, owner, 0) ||
        dev_alloc(c, (size_t)F2Q_UMI_CTR_WORDS, &u.ctr, owner, 0)) {
        free_all(c, owner);
        return fail(c, F2Q_ENOMEM, "no device memory for the UMI counters: " + c->err);
    }
    c->umi.dev.umis = u.umis; c->umi.dev.ctr = u.ctr; c->umi.fix_allocs = owner;
    return F2Q_OK;
}

// the linking launch (defaults and alternatives: DESIGN.md): threads per workgroup (F2Q_UMI_LINK_WG: whole waves, at most
// F2Q_UMI_LINK_THREADS), workgroups per CU at most (F2Q_UMI_LINK_GRID: 1 .. 4096), the lane-per-slot layout instead of the
// wave-cooperative one (F2Q_UMI_LINK=lane: A/B runs); anything else is the default.  g256: the grid of the slot-stride kernels
struct UmiGeom { uint32_t wg, g256, glink; bool by_lane; };
static UmiGeom umi_geometry(const f2q_ctx *c, uint64_t slots)
{
    uint32_t wg = F2Q_UMI_LINK_WG_DEFAULT, per_cu = F2Q_UMI_LINK_GRID_DEFAULT;
    { const char *e = getenv("F2Q_UMI_LINK_WG"); if (e && atol(e) >= 64 && atol(e) <= F2Q_UMI_LINK_THREADS && atol(e) % 64 == 0) wg = (uint32_t)atol(e); }
    { const char *e = getenv("F2Q_UMI_LINK_GRID"); if (e && atol(e) >= 1 && atol(e) <= 4096) per_cu = (uint32_t)atol(e); }
    const char *e = getenv("F2Q_UMI_LINK");
    return {wg, (uint32_t)std::min<uint64_t>((slots + 255) / 256, (uint64_t)c->n_cu * 8u),
            (uint32_t)std::min<uint64_t>((slots + wg - 1) / wg, (uint64_t)c->n_cu * per_cu), e && !strcmp(e, "lane")};
}

// The launches of a collapse, one after the other on the context's stream, the kernel boundary the only hand-off between
// them.  F2Q_TRACE=1: an event around each, ms[i] = the time of stage i once the last has ended (else ms[] stays as it is)
struct UmiStage { const char *name; std::function<void()> launch; };
static int umi_run_stages(f2q_ctx *c, const std::vector<UmiStage> &stages, float *ms)
{
    struct Events { std::vector<hipEvent_t> e; ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); } } ev;
    if (c->trace) { ev.e.assign(stages.size() + 1, nullptr); for (hipEvent_t &x : ev.e) HIPC(c, hipEventCreate(&x)); }
    for (size_t i = 0; i < stages.size(); i++) {
        if (c->trace) HIPC(c, hipEventRecord(ev.e[i], c->stream));
        stages[i].launch();
        HIPC(c, hipGetLastError());
        EC_POINT(c, stages[i].name);
    }
    if (!c->trace) return F2Q_OK;
    HIPC(c, hipEventRecord(ev.e.back(), c->stream));
    HIPC(c, hipEventSynchronize(ev.e.back()));
    for (size_t i = 0; i < stages.size(); i++) HIPC(c, hipEventElapsedTime(&ms[i], ev.e[i], ev.e[i + 1]));
    return F2Q_OK;
}

// UMIs of one feature at Hamming distance 1 joined, the groups counted (include/f2q.h).  A pass over the set after
// counting: parent[slots], molecules[n_features] and the edge counter are scratch from the device-memory cache and go
// back to it; the set, umis[] and the counters are only read, so the call changes nothing another call reads.
extern "C" int f2q_umi_collapse(f2q_ctx *c, int32_t dist, int64_t *molecules, int64_t extra[2])
{
    if (!c) return F2Q_EINVAL;
    if (c->raw_mode != RAW_UMI) return fail(c, F2Q_ESTATE, "not a UMI context: call f2q_set_umi first");
    if (dist != 0 && dist != 1) return fail(c, F2Q_EINVAL, "UMIs are collapsed at Hamming distance 1 (or 0: as they are)");
    HIPC(c, hipSetDevice(c->device));
    const double t0 = now_ms();
    const uint64_t nf = c->lib_h.n_features;
    std::vector<unsigned long long> h(nf + 1, 0ull);             // molecules, edges
    float ms[3] = {0, 0, 0};
    const UmiGeom g = umi_geometry(c, dist ? c->umi.set.n_slots : 0);     // (dist 0 launches nothing)
    const UmiDev &u = c->umi.dev;
    DevScope scratch(c);
    if (u.umis && u.slots && dist == 0) {                        // (nothing counted yet: all zero)
        if (nf) HIPC(c, hipMemcpyAsync(h.data(), u.umis, nf * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    } else if (u.umis && u.slots) {
        if (c->umi.set.n_slots > (1ull << 31)) return fail(c, F2Q_ENOMEM, "the UMI set has more than 2^31 slots: too large to collapse");
        uint32_t *parent = nullptr; unsigned long long *mol = nullptr;
        if (dev_alloc(c, (size_t)c->umi.set.n_slots, &parent, scratch.v) || dev_alloc(c, (size_t)nf + 1, &mol, scratch.v, 0))
            return fail(c, F2Q_ENOMEM, "no device memory to collapse a UMI set of " + std::to_string(c->umi.set.n_slots) + " slots: " + c->err);
        const std::vector<UmiStage> stages = {
            {"k_umi_uf_init", [&] { hipLaunchKernelGGL(k_umi_uf_init, dim3(g.g256), dim3(256), 0, c->stream, parent, (unsigned long long)c->umi.set.n_slots); }},
            {"k_umi_link", [&] {
                if (g.by_lane) hipLaunchKernelGGL(k_umi_link_lane, dim3(g.glink), dim3(g.wg), 0, c->stream, u, parent, mol + nf);
                else hipLaunchKernelGGL(k_umi_link<false>, dim3(g.glink), dim3(g.wg), 0, c->stream, u, parent, (uint32_t *)nullptr, mol + nf); }},
            {"k_umi_roots", [&] { hipLaunchKernelGGL(k_umi_roots, dim3(g.g256), dim3(256), 0, c->stream, u, parent, mol); }}};
        if (int rc = umi_run_stages(c, stages, ms)) return rc;
        HIPC(c, hipMemcpyAsync(h.data(), mol, (nf + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    }
    unsigned long long ctr[F2Q_UMI_CTR_WORDS];
    if (int rc = pairset_read_ctr(c, c->umi.set, ctr)) return rc;
    unsigned long long total = 0;
    for (uint64_t i = 0; i < nf; i++) { total += h[i]; if (molecules) molecules[i] = (int64_t)h[i]; }
    if (extra) { extra[0] = (int64_t)ctr[F2Q_UMI_HELD]; extra[1] = (int64_t)h[nf]; }
    if (c->trace) fprintf(stderr, "[f2q trace] UMI collapse: %llu pairs, %llu edges, %llu molecules, %.3f ms (union-find init %.3f, link %.3f, roots %.3f; %s, %u x %u)\n",
                          ctr[F2Q_UMI_HELD], h[nf], total, now_ms() - t0, ms[0], ms[1], ms[2], g.by_lane ? "lane" : "wave", g.glink, g.wg);
    return F2Q_OK;
}

// the wrap of a 32-bit count excluded on the host: no pair can have 2^32 reads while the context has counted fewer
static int umi_reads_ready(f2q_ctx *c, const char *who, unsigned long long ctr[F2Q_UMI_CTR_WORDS])
{
    if (c->raw_mode != RAW_UMI) return fail(c, F2Q_ESTATE, "not a UMI context: call f2q_set_umi first");
    if (!c->umi.set.keep_reads) return fail(c, F2Q_ESTATE, std::string(who) + " needs the reads per pair: call f2q_set_umi_reads before counting");
    HIPC(c, hipSetDevice(c->device));
    if (int rc = pairset_read_ctr(c, c->umi.set, ctr)) return rc;
    if (ctr[F2Q_UMI_READS] >= (1ull << 32))
        return fail(c, F2Q_EUNSUPPORTED, std::string(who) + ": 2^32 or more reads with a valid UMI -- a pair's 32-bit count may have wrapped");
    return F2Q_OK;
}

// The directional rule of UMI-tools over the same set (include/f2q.h; the rule as it is computed: DESIGN.md).  Four
// launches; parent[slots], dom[slots], molecules[n_features] and three counters are scratch from the device-memory cache.
// The set, reads[], umis[] and the counters are only read.
extern "C" int f2q_umi_collapse_directional(f2q_ctx *c, int64_t *molecules, int64_t extra[4])
{
    if (!c) return F2Q_EINVAL;
    unsigned long long ctr[F2Q_UMI_CTR_WORDS];
    if (int rc = umi_reads_ready(c, "f2q_umi_collapse_directional", ctr)) return rc;
    const double t0 = now_ms();
    const uint64_t nf = c->lib_h.n_features;
    std::vector<unsigned long long> h(nf + 3, 0ull);             // molecules, edges, flagged slots, reads
    float ms[4] = {0, 0, 0, 0};
    const UmiGeom g = umi_geometry(c, c->umi.set.n_slots);
    const UmiDev &u = c->umi.dev;
    DevScope scratch(c);
    if (u.umis && u.slots && u.reads) {                          // (nothing counted yet: all zero)
        if (c->umi.set.n_slots > (1ull << 31)) return fail(c, F2Q_ENOMEM, "the UMI set has more than 2^31 slots: too large to collapse");
        uint32_t *parent = nullptr, *dom = nullptr; unsigned long long *mol = nullptr;
        if (dev_alloc(c, (size_t)c->umi.set.n_slots, &parent, scratch.v) || dev_alloc(c, (size_t)c->umi.set.n_slots, &dom, scratch.v, 0) ||
            dev_alloc(c, (size_t)nf + 3, &mol, scratch.v, 0))
            return fail(c, F2Q_ENOMEM, "no device memory to collapse a UMI set of " + std::to_string(c->umi.set.n_slots) + " slots: " + c->err);
        const std::vector<UmiStage> stages = {
            {"k_umi_uf_init", [&] { hipLaunchKernelGGL(k_umi_uf_init, dim3(g.g256), dim3(256), 0, c->stream, parent, (unsigned long long)c->umi.set.n_slots); }},
            {"k_umi_link_dir", [&] { hipLaunchKernelGGL(k_umi_link<true>, dim3(g.glink), dim3(g.wg), 0, c->stream, u, parent, dom, mol + nf); }},
            {"k_umi_dir_spread", [&] { hipLaunchKernelGGL(k_umi_dir_spread, dim3(g.g256), dim3(256), 0, c->stream, u, (const uint32_t *)parent, dom); }},
            {"k_umi_dir_roots", [&] { hipLaunchKernelGGL(k_umi_dir_roots, dim3(g.g256), dim3(256), 0, c->stream, u, (const uint32_t *)parent, (const uint32_t *)dom, mol, mol + nf + 1); }}};
        if (int rc = umi_run_stages(c, stages, ms)) return rc;
        HIPC(c, hipMemcpyAsync(h.data(), mol, (nf + 3) * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipStreamSynchronize(c->stream));
    }
    unsigned long long total = 0;
    for (uint64_t i = 0; i < nf; i++) { total += h[i]; if (molecules) molecules[i] = (int64_t)h[i]; }
    if (extra) { extra[0] = (int64_t)ctr[F2Q_UMI_HELD]; extra[1] = (int64_t)h[nf]; extra[2] = (int64_t)h[nf + 1]; extra[3] = (int64_t)h[nf + 2]; }
    if (c->trace) fprintf(stderr, "[f2q trace] UMI collapse directional: %llu pairs, %llu edges, %llu dominated, %llu molecules, %llu reads, %.3f ms (union-find init %.3f, link %.3f, spread %.3f, roots %.3f; wave, %u x %u)\n",
                          ctr[F2Q_UMI_HELD], h[nf], h[nf + 1], total, h[nf + 2], now_ms() - t0, ms[0], ms[1], ms[2], ms[3], g.glink, g.wg);
    return F2Q_OK;
}

// every pair the set holds with its reads, sorted by (feature, codes): the table copied and filtered on the host (no hot path)
extern "C" int f2q_umi_pairs(f2q_ctx *c, uint64_t cap, uint64_t *n, uint32_t *feature, uint32_t *codes, uint32_t *reads)
{
    if (!c || !n) return F2Q_EINVAL;
    unsigned long long ctr[F2Q_UMI_CTR_WORDS];
    if (int rc = umi_reads_ready(c, "f2q_umi_pairs", ctr)) return rc;
    *n = ctr[F2Q_UMI_HELD];
    if (!feature && !codes && !reads) return F2Q_OK;
    if (cap < *n) return fail(c, F2Q_EINVAL, "f2q_umi_pairs: room for " + std::to_string(cap) + " pairs, the set holds " + std::to_string(*n));
    if (!*n || !c->umi.dev.slots || !c->umi.dev.reads) return F2Q_OK;
    std::vector<unsigned long long> words;                       // 12 bytes per slot on the host: a failure is F2Q_ENOMEM, not an exception
    std::vector<uint32_t> cnt;
    std::vector<std::pair<unsigned long long, uint32_t>> held;
    try { words.resize(c->umi.set.n_slots); cnt.resize(c->umi.set.n_slots); held.reserve((size_t)*n); }
    catch (const std::bad_alloc &) { return fail(c, F2Q_ENOMEM, "no host memory to copy a UMI set of " + std::to_string(c->umi.set.n_slots) + " slots"); }
    HIPC(c, hipMemcpyAsync(words.data(), c->umi.dev.slots, c->umi.set.n_slots * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(cnt.data(), c->umi.dev.reads, c->umi.set.n_slots * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    uint64_t occupied = 0;
    for (uint64_t i = 0; i < c->umi.set.n_slots; i++) if (words[i] != KEY_EMPTY && occupied++ < *n) held.emplace_back(words[i], cnt[i]);      // (never past the reserve)
    if (occupied != *n) return fail(c, F2Q_EHIP, "the UMI set holds " + std::to_string(occupied) + " pairs, its counter says " + std::to_string(*n));
    std::sort(held.begin(), held.end());                         // the word is (feature << 32) | codes
    for (size_t i = 0; i < held.size(); i++) {
        if (feature) feature[i] = (uint32_t)(held[i].first >> 32);
        if (codes) codes[i] = (uint32_t)held[i].first;
        if (reads) reads[i] = held[i].second;
    }
    return F2Q_OK;
}

// The raw records of a view, one launch: the byte-exact routine per record, in the kernel of the context's mode -- the same
// road with the (feature, UMI) set, the barcode verdict and the matrix, the reverse strand, the window at n + 1 starts, the
// indel trial of the unassigned reads, or the part verdicts and the recombinant set.
static int launch_raw(f2q_ctx *c, const RawBlock &rbv, Accum &acc, uint32_t &launches)
{
    int rc;
    if ((rc = acc_ready(c))) return rc;                          // the raw-record kernels add to the accumulators directly
    RawBlock rb = rbv;
    rb.first_index += c->reads_seen;
    const uint64_t wg = (rb.n + F2Q_GEN_THREADS - 1) / F2Q_GEN_THREADS;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(wg, (uint64_t)c->n_cu * 64u);
    // kern(run, lib, tail...) over the records, with `shmem` bytes of dynamic LDS
    auto launch = [&](const char *name, size_t shmem, auto kern, const auto &...tail) -> int {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(F2Q_GEN_THREADS), shmem, c->stream, c->run_d, c->lib_d, tail...);
        HIPC(c, hipGetLastError());
        launches++;
        EC_POINT(c, name);
        return F2Q_OK;
    };
    switch (c->raw_mode) {
        case RAW_NONE:
            return launch("k_count_general", 0, rb.len1 ? k_count_general<true> : k_count_general<false>, c->ec, rb, acc);
        case RAW_UMI: {
            if ((rc = umi_counters(c)) || (rc = pairset_reserve(c, c->umi.set, rb.n))) return rc;
            const UmiDev &u = c->umi.dev;
            const bool keep = u.reads != nullptr;
            if (c->umi.hdr_sep) {                                // the UMI comes from the header (f2q_set_umi_header): rb.hdr_umi
                if (!rb.hdr_umi) return fail(c, F2Q_ESTATE, "a block without header UMIs on a header-UMI context");
                if (!rb.len1) return launch("k_count_umi (header)", 0, keep ? k_count_umi<true, true> : k_count_umi<false, true>, c->ec, rb, acc, u);
                return launch("k_count_umi_pair (header)", 0, keep ? k_count_umi_pair<true, F2Q_UMI_PAIR_STAGE_DEFAULT, true> : k_count_umi_pair<false, F2Q_UMI_PAIR_STAGE_DEFAULT, true>, c->ec, rb, acc, u);
            }
            if (!rb.len1) return launch("k_count_umi", 0, keep ? k_count_umi<true> : k_count_umi<false>, c->ec, rb, acc, u);
            // merged pairs (f2q_set_umi_paired): a pair is one record
            if (!u.len1 && !u.len2) return fail(c, F2Q_ESTATE, "a block of pairs on a single-read UMI context");
            if (c->umi.pair_stage) return launch("k_count_umi_pair", 0, keep ? k_count_umi_pair<true, true> : k_count_umi_pair<false, true>, c->ec, rb, acc, u);
            return launch("k_count_umi_pair", 0, keep ? k_count_umi_pair<true, false> : k_count_umi_pair<false, false>, c->ec, rb, acc, u);
        }
        case RAW_DEMUX: {
            if ((rc = demux_alloc(c))) return rc;                // (only after an allocation that failed: a retry)
            const DemuxDev &d = c->demux.dev;
            const bool lds = c->demux.lds_table;
            const size_t shmem = (lds ? ((size_t)d.mask + 1) * 8 : 0) + ((size_t)d.n + 1) * 5 * 4;
            // the most any context can ask for, so that dyn_lds sets it once: the attribute belongs to the kernel, not to the context
            const size_t most = (lds ? (size_t)F2Q_DEMUX_LDS_SLOTS * 8 : 0) + ((size_t)F2Q_DEMUX_MAXN + 1) * 5 * 4;
            if ((rc = dyn_lds(c, lds ? (const void *)k_count_demux<true> : (const void *)k_count_demux<false>, most))) return rc;
            return launch("k_count_demux", shmem, lds ? k_count_demux<true> : k_count_demux<false>, c->ec, rb, acc, d);
        }
        case RAW_STRAND: {
            if ((rc = strand_alloc(c))) return rc;               // (only after an allocation that failed: a retry)
            const bool both = c->strand.mode == F2Q_STRAND_BOTH;
            return launch(both ? "k_count_strand<both>" : "k_count_strand<rev>", 0, both ? k_count_strand<true> : k_count_strand<false>, c->ec, rb, acc, c->strand.dev);
        }
        case RAW_STAGGER:
            return launch("k_count_stagger", 0, k_count_stagger, rb, acc, c->stagger.dev);
        case RAW_INDEL:
            if (!c->indel.dev.del_counts && (rc = indel_install(c, true))) return rc;      // (only after an allocation that failed: a retry)
            if (!c->indel.dev.del_counts) return fail(c, F2Q_ESTATE, "an indel context without its table: f2q_set_features failed");
            return launch("k_count_indel", 0, k_count_indel, c->ec, rb, acc, c->indel.dev);
        case RAW_PARTS:
            if (!c->parts.dev.counts) return fail(c, F2Q_ESTATE, "a parts context without its tables: f2q_set_features failed");
            if ((rc = pairset_reserve(c, c->parts.set, rb.n))) return rc;
            return launch(rb.len1 ? "k_count_parts<paired>" : "k_count_parts", 0, rb.len1 ? k_count_parts<true> : k_count_parts<false>, c->ec, rb, acc, c->parts.dev);
    }
    return fail(c, F2Q_ESTATE, "no such raw-record mode");
}

// one set of launches over a view of a block (all of it in Counter mode, a step of it in Extract+Count mode)
static int launch_view(f2q_ctx *c, const PackedBlock &pb, const RawBlock &rbv, Accum &acc, uint32_t &launches)
{
    int rc = F2Q_OK;
    if (pb.n_tiles) {
        c->last_path = choose_path(c, pb);
        // k_count_fixed4_lds and k_count_fixed4 meet the accumulators in k_reduce_slabs only, which consumes a pending
        // clear by storing; the kernels of every other path add to them (if only for a read their slow routine decides)
        const bool slab_only = c->prm.mode == 0 && c->lib_h.n_features &&
                               (c->last_path == F2Q_PATH_FIXED_LDS || c->last_path == F2Q_PATH_MULTI_LDS || c->last_path == F2Q_PATH_FIXED_PACKED);
        if (!slab_only && (rc = acc_ready(c))) return rc;
    }
    if (pb.n_tiles) switch (c->last_path) {
        case F2Q_PATH_PAIRS:        rc = launch_pairs(c, pb, acc, launches); break;
        case F2Q_PATH_ANCHOR:       rc = launch_anchor(c, pb, acc, launches); break;
        case F2Q_PATH_ANCHOR_LDS:   rc = launch_anchor_lds(c, pb, acc, launches); break;
        case F2Q_PATH_EXTRACT:      rc = pb.planar_nw ? launch_anchor(c, pb, acc, launches) : launch_extract_fixed(c, pb, acc, launches); break;
        case F2Q_PATH_MULTI_LDS:    rc = launch_fixed_lds(c, pb, acc, launches, true); break;
        case F2Q_PATH_MULTI:        rc = launch_multi(c, pb, acc, launches); break;
        case F2Q_PATH_FIXED_PART:   rc = launch_part(c, pb, acc, launches); break;
        case F2Q_PATH_FIXED_LDS:    rc = launch_fixed_lds(c, pb, acc, launches, false); break;
        case F2Q_PATH_FIXED_PACKED: rc = launch_fixed_packed(c, pb, acc, launches); break;
        default:                    rc = launch_fixed_v1(c, pb, acc, launches); break;
    }
    if (rc || !rbv.n) return rc;
    return launch_raw(c, rbv, acc, launches);
}

// ---- Extract+Count, anchored tiles, hot keys in LDS (EcHot, k_extract_anchor_hot) ---------------------------------
static int hot_arrays(f2q_ctx *c)
{
    if (c->hot.keys) return F2Q_OK;
    int rc;
    if ((rc = dev_alloc(c, (size_t)F2Q_HOT_SLOTS, &c->hot.keys, c->hot_allocs, 0xFF))) return rc;
    if ((rc = dev_alloc(c, (size_t)F2Q_HOT_SLOTS, &c->hot.slot, c->hot_allocs))) return rc;
    if ((rc = dev_alloc(c, (size_t)2, &c->hot.meta, c->hot_allocs, 0))) return rc;
    return dev_alloc(c, (size_t)F2Q_HOT_CAND, &c->hot.cand, c->hot_allocs);
}
// the set from the candidates the learning launches noted
static int hot_build(f2q_ctx *c)
{
    int rc = hot_arrays(c);
    if (rc) return rc;
    HIPC(c, hipMemsetAsync(c->hot.keys, 0xFF, (size_t)F2Q_HOT_SLOTS * 8, c->stream));
    HIPC(c, hipMemsetAsync(c->hot.meta, 0, 16, c->stream));
    if (c->ec.k64_slots) {
        hipLaunchKernelGGL(k_ec_hot_build, dim3((F2Q_HOT_CAP + 255) / 256), dim3(256), 0, c->stream, c->ec, c->hot);
        HIPC(c, hipGetLastError());
        EC_POINT(c, "hot set: build");
    }
    c->hot_valid = true;
    return F2Q_OK;
}

// the raw records of a block on the second stream (after ev_aux0: tables reserved, block resident)
static int launch_aux_general(f2q_ctx *c, const f2q_block *b, Accum &acc, uint32_t &launches)
{
    HIPC(c, hipStreamWaitEvent(c->aux_stream, c->ev_aux0, 0));
    RawBlock rb = b->rb;
    rb.first_index += c->reads_seen;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((rb.n + F2Q_GEN_THREADS - 1) / F2Q_GEN_THREADS, (uint64_t)c->n_cu * 32u);
    hipLaunchKernelGGL(k_count_general<false>, dim3(grid), dim3(F2Q_GEN_THREADS), 0, c->aux_stream, c->run_d, c->lib_d, c->ec, rb, acc);
    HIPC(c, hipGetLastError());
    launches++;
    c->aux_busy = true;
    return F2Q_OK;
}

// reads the Extract+Count counters into ctr (after the stream's work so far); a table that overflowed fails the call
static int ec_counters(f2q_ctx *c, unsigned long long ctr[F2Q_CTR_WORDS])
{
    HIPC(c, hipMemcpyAsync(ctr, c->ec.ctr, F2Q_CTR_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    if (ctr[2]) return fail(c, F2Q_ENOMEM, "Extract+Count table overflow (internal sizing error, code " + std::to_string(ctr[2]) + ")");
    return F2Q_OK;
}
// an Extract+Count block whose packed tiles take the hot-key kernels: anchored tiles of one pair (not the 161 .. 320-base
// instantiation) and fixed-window tiles
static bool ec_hot_path(const f2q_ctx *c, const f2q_block *b)
{
    const PackedBlock &pb = b->pb;
    return pb.n_tiles && !c->no_hot && !c->plan.multi_pair && (!pb.planar_nw || (pb.len != nullptr && pb.planar_nw != 10));
}

// one launch of the hot-key kernel over a view of the block's anchored tiles (it starts slot_base slots into the
// block); the tables have room (the caller reserved).  learning: the hot set is not built yet, the kernel runs with an
// empty one and notes the keys that come up F2Q_HOT_MINCOUNT times.  ctr: the counters after the launch.
static int launch_hot(f2q_ctx *c, const PackedBlock &v, uint64_t slot_base, Accum &acc, uint32_t &launches, bool learning,
                      unsigned long long ctr[F2Q_CTR_WORDS], const f2q_block *aux_block)
{
    int rc = hot_arrays(c);
    if (rc) return rc;
    c->last_path = F2Q_PATH_EXTRACT;                             // (these launches do not go through launch_view)
    if (learning) HIPC(c, hipMemsetAsync(c->hot.keys, 0xFF, (size_t)F2Q_HOT_SLOTS * 8, c->stream));   // an empty set
    const size_t shmem = (size_t)F2Q_HOT_SLOTS * 12;             // key words + counters
    if (!v.planar_nw) {
        // fixed window: one wave per tile
        const uint32_t wgs = (v.n_tiles + F2Q_FH_WAVES - 1) / F2Q_FH_WAVES;
        uint32_t fgrid = std::min<uint32_t>(wgs, (uint32_t)c->n_cu);
        if (c->lt_max_wgs) fgrid = std::min<uint32_t>(fgrid, c->lt_max_wgs);
        auto kern = learning ? k_extract_fixed4_hot<true> : k_extract_fixed4_hot<false>;
        if ((rc = dyn_lds(c, (const void *)kern, shmem))) return rc;
        hipLaunchKernelGGL(kern, dim3(fgrid), dim3(F2Q_FH_THREADS), shmem, c->stream, c->run_d, c->ec, c->hot, v, acc, c->reads_seen,
                           c->defer_d, slot_base, (uint64_t)c->defer_cap);
    } else {
        const uint32_t groups = (v.n_tiles + F2Q_HOT_GROUPS - 1) / F2Q_HOT_GROUPS;
        uint32_t grid = std::min<uint32_t>(groups, (uint32_t)c->n_cu);
        if (c->lt_max_wgs) grid = std::min<uint32_t>(grid, c->lt_max_wgs);
        anchored_geom(v.planar_nw, c->plan.kb, same_q(c->run_h), [&](auto NW, auto KB, auto SQ) {
            auto kern = learning ? k_extract_anchor_hot<NW, KB, SQ, true> : k_extract_anchor_hot<NW, KB, SQ, false>;
            if ((rc = dyn_lds(c, (const void *)kern, shmem))) return;
            hipLaunchKernelGGL(kern, dim3(grid), dim3(F2Q_HOT_THREADS), shmem, c->stream, c->run_d, c->ec, c->hot, v, acc,
                               c->reads_seen, c->defer_d, slot_base, (uint64_t)c->defer_cap);
        });
        if (rc) return rc;
    }
    HIPC(c, hipGetLastError());
    launches++;
    if (aux_block && (rc = launch_aux_general(c, aux_block, acc, launches))) return rc;
    EC_POINT(c, learning ? "k_extract_anchor_hot (learning)" : "k_extract_anchor_hot");
    return ec_counters(c, ctr);
}

// the reads the launches over a block set aside (ctr: the counters as just read): windows the single-word table cannot
// hold go to the byte-string table from the planes, the rest through the byte-exact routine
static int hot_aside(f2q_ctx *c, const PackedBlock &blk, Accum &acc, uint32_t &launches, const unsigned long long ctr[F2Q_CTR_WORDS])
{
    const unsigned long long n_def = ctr[F2Q_CTR_ASIDE], n_slow = ctr[F2Q_CTR_ASIDE_SLOW];
    if (!n_def) return F2Q_OK;
    // the raw records' kernel may still be adding entries: the counters read after the launch say too little then
    const unsigned long long *known = ctr;
    if (c->aux_busy) { HIPC(c, hipStreamSynchronize(c->aux_stream)); c->aux_busy = false; known = nullptr; }
    int rc = ec_reserve(c, n_slow, n_def, n_def * ((uint64_t)blk.rmax + F2Q_MAX_ITER), known);
    if (rc) return rc;
    const uint32_t g = (uint32_t)std::min<uint64_t>((n_def + 255) / 256, (uint64_t)c->n_cu * 8u);
    if (n_def > n_slow) {
        hipLaunchKernelGGL(k_ec_deferred_keys, dim3(g), dim3(256), 0, c->stream, c->ec, blk, acc, c->reads_seen, c->defer_d);
        HIPC(c, hipGetLastError());
        launches++;
        EC_POINT(c, "k_ec_deferred_keys");
    }
    if (n_slow && !blk.planar_nw) {
        hipLaunchKernelGGL(k_ec_deferred_fixed, dim3(g), dim3(256), 0, c->stream, c->run_d, c->ec, blk, acc, c->reads_seen, c->defer_d);
        HIPC(c, hipGetLastError());
        launches++;
        EC_POINT(c, "k_ec_deferred_fixed");
    } else if (n_slow) {
        hipLaunchKernelGGL(k_ec_deferred_slow, dim3(g), dim3(256), 0, c->stream, c->run_d, c->lib_d, c->ec, blk, acc, c->reads_seen, c->defer_d);
        HIPC(c, hipGetLastError());
        launches++;
        EC_POINT(c, "k_ec_deferred_slow");
    }
    return F2Q_OK;
}

static int launch_block(f2q_ctx *c, const f2q_block *b, f2q_timing *t, hipEvent_t k0 = nullptr, hipEvent_t k1 = nullptr)
{
    if (!k0) { k0 = c->ev_k0; k1 = c->ev_k1; }          // (a queued step brings its own pair)
    if (c->prm.mode == 0 && !c->have_lib) return fail(c, F2Q_ESTATE, "f2q_set_features must be called before counting in Counter mode");
    if (c->raw_mode != RAW_NONE) if (int rc = raw_mode_block(c, b)) return rc;
    c->counted = true;
    Accum acc{c->acc_d, c->acc_d + (c->acc_n - 5), nullptr, nullptr, nullptr, nullptr, c->carry_d};
#ifdef F2Q_STAMP
    static unsigned long long *stamp_d = nullptr;
    if (!stamp_d) { (void)hipMalloc((void **)&stamp_d, 64); (void)hipMemset(stamp_d, 0, 64); }
    acc.stamp = stamp_d;
#endif
    uint32_t launches = 0;
    HIPC(c, hipEventRecord(k0, c->stream));
    c->ec_gen++;
    if (c->prm.mode == 0) {
        int rc = launch_view(c, b->pb, b->rb, acc, launches);
        if (rc) return rc;
    } else if (b->n_reads) {
        if (int rc = acc_ready(c)) return rc;            // every Extract+Count kernel adds its five counters directly
        // Extract+Count: the tables must have room for "every read of the launch is a new key".  Sizing them for the
        // whole block (50 M reads -> 2^28 slots) makes the table many GiB and every probe a DRAM access, so the block
        // is walked in steps of F2Q_EC_STEP reads: room for one step beyond the keys already there is enough, and the
        // tables grow (device rehash) only when the number of distinct keys does.
        uint64_t step = (uint64_t)8 << 20;
        { const char *e = getenv("F2Q_EC_STEP"); if (e && atol(e) >= F2Q_TILE) step = (uint64_t)atol(e); }
        const uint32_t tiles_per = (uint32_t)std::max<uint64_t>(1, step / F2Q_TILE);
        const RawBlock none{};
        auto view_of = [&](uint32_t t0, uint32_t nt) {
            PackedBlock v = b->pb;
            v.n_tiles = nt; v.n_slots = (uint64_t)nt * F2Q_TILE;
            v.bases += (size_t)t0 * v.wb * F2Q_TILE; v.qual += (size_t)t0 * v.wq * F2Q_TILE;
            if (v.len) v.len += (size_t)t0 * F2Q_TILE;
            if (v.index) v.index += (size_t)t0 * F2Q_TILE; else v.first_index += (uint64_t)t0 * F2Q_TILE;
            return v;
        };
        const bool hot_path = ec_hot_path(c, b);
        if (hot_path) {
            // anchored tiles: hot keys in LDS.  The first hot_learn reads of a sample go through the same kernel with an
            // empty hot set (every key takes the table's insert); then the set is built and serves the rest of the sample.
            // The raw records are decided on a second stream while the packed tiles are counted.
            const uint64_t n = (uint64_t)b->pb.n_tiles * F2Q_TILE;
            const uint64_t to_learn = c->hot_valid || c->ec_learned >= c->hot_learn ? 0 : std::min<uint64_t>(n, c->hot_learn - c->ec_learned);
            unsigned long long ctr[F2Q_CTR_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
            int rc;
            if (c->ec.ctr && (rc = ec_counters(c, ctr))) return rc;
            // new single-word keys to expect: at the rate the sample has shown once the learning reads are in (a table that
            // fills up all the same only moves reads to the deferred pass), a guess of one key per six reads before that
            auto expect_of = [&](uint64_t reads) {
                const double rate = std::min(1.0, (double)ctr[3] / (double)std::max<uint64_t>(c->ec_learned, 1));
                return std::min<uint64_t>(reads, (uint64_t)(rate * (double)reads) + 4096);
            };
            const uint64_t aside = 4096 + n / 2048;                                 // reads the packed kernel may set aside
            const uint64_t raw_bytes = b->raw_key_bytes + b->rb.n * F2Q_MAX_ITER + aside * ((uint64_t)b->pb.rmax + F2Q_MAX_ITER);
            if ((rc = ec_reserve(c, (to_learn ? to_learn + (n - to_learn) / 6 : expect_of(n)) + b->rb.n + aside, b->rb.n + aside, raw_bytes, ctr))) return rc;
            // the list of reads set aside: room for every slot of the block, cleared once per block
            if ((rc = grow_buf(c, &c->defer_d, c->defer_cap, n, false))) return rc;
            HIPC(c, hipMemsetAsync(c->ec.ctr + F2Q_CTR_ASIDE, 0, 16, c->stream));
            uint32_t t0 = 0;
            if (to_learn) {
                const uint32_t nt = (uint32_t)((to_learn + F2Q_TILE - 1) / F2Q_TILE);
                if ((rc = launch_hot(c, view_of(0, nt), 0, acc, launches, true, ctr, nullptr))) return rc;
                c->ec_learned += (uint64_t)nt * F2Q_TILE;
                t0 = nt;
                // the sample's own rate replaces the guess (the reads set aside so far are still to come: `aside` covers them)
                if (t0 < b->pb.n_tiles && (rc = ec_reserve(c, expect_of(n - (uint64_t)t0 * F2Q_TILE) + b->rb.n + aside, b->rb.n + aside, raw_bytes, ctr))) return rc;
            }
            if (t0 < b->pb.n_tiles && !c->hot_valid && (rc = hot_build(c))) return rc;
            if (b->rb.n) {
                if (!c->aux_stream) {
                    HIPC(c, hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking));
                    HIPC(c, hipEventCreateWithFlags(&c->ev_aux0, hipEventDisableTiming));
                    HIPC(c, hipEventCreateWithFlags(&c->ev_aux1, hipEventDisableTiming));
                }
                HIPC(c, hipEventRecord(c->ev_aux0, c->stream));                     // the tables and the block are ready
            }
            // the long launch goes first; the raw records' kernel fills the wave slots it leaves free
            if (t0 < b->pb.n_tiles) {
                if ((rc = launch_hot(c, view_of(t0, b->pb.n_tiles - t0), (uint64_t)t0 * F2Q_TILE, acc, launches, false, ctr, b->rb.n ? b : nullptr))) return rc;
            } else if (b->rb.n && (rc = launch_aux_general(c, b, acc, launches))) return rc;
            if ((rc = hot_aside(c, view_of(0, b->pb.n_tiles), acc, launches, ctr))) return rc;
            if (c->aux_busy) {                                                       // join: the block is done when both streams are
                HIPC(c, hipEventRecord(c->ev_aux1, c->aux_stream));
                HIPC(c, hipStreamWaitEvent(c->stream, c->ev_aux1, 0));
                c->aux_busy = false;
            }
        } else
        for (uint32_t t0 = 0; t0 < b->pb.n_tiles; t0 += tiles_per) {
            const PackedBlock v = view_of(t0, std::min<uint32_t>(tiles_per, b->pb.n_tiles - t0));
            // packed reads give single-window keys of at most rmax bytes (several pairs: one window each, at most F2Q_PAIRS_KEYMAX in all)
            const uint64_t key_max = c->plan.multi_pair ? (uint64_t)F2Q_PAIRS_KEYMAX : (uint64_t)v.rmax + F2Q_MAX_ITER;
            int rc = ec_reserve(c, v.n_slots, v.n_slots, v.n_slots * key_max);
            if (rc) return rc;
            if ((rc = launch_view(c, v, none, acc, launches))) return rc;
        }
        const PackedBlock nop{};
        for (uint64_t r0 = 0; r0 < b->rb.n && !hot_path; r0 += step) {
            RawBlock v = b->rb;
            v.n = std::min<uint64_t>(step, b->rb.n - r0);
            v.off += r0; v.len += r0; v.qlen += r0;
            if (v.qoff) v.qoff += r0;
            if (v.len1) { v.len1 += r0; v.qlen1 += r0; }
            if (v.index) v.index += r0; else v.first_index += r0;
            // no key is longer than its record's bytes + separators (block-wide bound: the arena is never cleared)
            int rc = ec_reserve(c, v.n, v.n, b->raw_key_bytes + v.n * F2Q_MAX_ITER);
            if (rc) return rc;
            if ((rc = launch_view(c, nop, v, acc, launches))) return rc;
        }
    }
    HIPC(c, hipEventRecord(k1, c->stream));
    c->reads_seen += b->n_reads;
#ifdef F2Q_STAMP
    { unsigned long long h[8]; (void)hipStreamSynchronize(c->stream); (void)hipMemcpy(h, acc.stamp, 64, hipMemcpyDeviceToHost);
      (void)hipMemset(acc.stamp, 0, 64);
      unsigned long long tot = 0;
      for (int i = 0; i < 8; i++) tot += h[i];
      if (tot) {
          fprintf(stderr, "[stamp]");
          for (int i = 0; i < 8; i++) if (h[i]) fprintf(stderr, " phase %d %.1f%%", i, 100.0 * h[i] / tot);
          fprintf(stderr, "  (%.0f clock ticks/wave-tile)\n", (double)tot / ((double)b->pb.n_tiles * 4));
      } }
#endif
    if (t) {
        HIPC(c, hipEventSynchronize(k1));
        float ms = 0;
        HIPC(c, hipEventElapsedTime(&ms, k0, k1));
        t->kernel_ms = ms; t->reads = b->n_reads; t->general_reads = b->n_general;
        t->fast_reads = b->n_reads - b->n_general; t->launches = launches; t->path = c->last_path;
    }
    if (c->prm.mode == 1 && b->n_reads && !ec_hot_path(c, b)) {
        // (the hot-key path has looked at the counters after its last launch; what its deferred passes could still
        // report is seen by the next call that reads them)
        unsigned long long ctr[F2Q_CTR_WORDS];
        return ec_counters(c, ctr);
    }
    return F2Q_OK;
}

static void timing_add(f2q_timing &sum, const f2q_timing &one)
{
    sum.kernel_ms += one.kernel_ms; sum.total_ms += one.total_ms; sum.reads += one.reads;
    sum.fast_reads += one.fast_reads; sum.general_reads += one.general_reads; sum.launches += one.launches;
    if (one.path) sum.path = one.path;
}

// the ev_a / ev_b bracket of a counting call: ev_a was recorded on c->stream when the call began; *t = sum, with
// total_ms the event time from there to now
static int timing_close(f2q_ctx *c, f2q_timing *t, const f2q_timing &sum)
{
    if (!t) return F2Q_OK;
    hipError_t e = hipEventRecord(c->ev_b, c->stream);
    if (e == hipSuccess) e = hipEventSynchronize(c->ev_b);
    float ms = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, c->ev_a, c->ev_b);
    if (e != hipSuccess) return fail(c, F2Q_EHIP, hipGetErrorString(e));
    *t = sum; t->total_ms = ms;
    return F2Q_OK;
}

extern "C" int f2q_count_resident(f2q_ctx *c, const f2q_block *b, f2q_timing *t)
{
    if (!c || !b) return F2Q_EINVAL;
    HIPC(c, hipSetDevice(c->device));
    if (t) { memset(t, 0, sizeof *t); HIPC(c, hipEventRecord(c->ev_a, c->stream)); }
    int rc = launch_block(c, b, t);
    if (rc) return rc;
    return t ? timing_close(c, t, *t) : F2Q_OK;
}

extern "C" int f2q_count_resident_queued(f2q_ctx *c, const f2q_block *b)
{
    if (!c || !b) return F2Q_EINVAL;
    HIPC(c, hipSetDevice(c->device));
    while (c->q_ev.size() < 2 * ((size_t)c->q_n + 1)) {
        hipEvent_t e = nullptr;
        HIPC(c, hipEventCreate(&e));
        c->q_ev.push_back(e);
    }
    int rc = launch_block(c, b, nullptr, c->q_ev[2 * (size_t)c->q_n], c->q_ev[2 * (size_t)c->q_n + 1]);
    if (rc) return rc;
    c->q_n++;
    return F2Q_OK;
}

extern "C" int f2q_queued_times(f2q_ctx *c, float *kernel_ms, uint32_t cap, uint32_t *n)
{
    if (!c || !n) return F2Q_EINVAL;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    *n = c->q_n;
    for (uint32_t i = 0; i < c->q_n && i < cap && kernel_ms; i++)
        HIPC(c, hipEventElapsedTime(&kernel_ms[i], c->q_ev[2 * (size_t)i], c->q_ev[2 * (size_t)i + 1]));
    c->q_n = 0;
    return F2Q_OK;
}

extern "C" void f2q_block_free(f2q_ctx *c, f2q_block *b)
{
    if (!b) return;
    if (c) { (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->stream); }
    free_all(c, b->allocs);
    delete b;
}

extern "C" int f2q_block_info(const f2q_block *b, uint64_t *n_reads, uint64_t *n_general, uint64_t *device_bytes)
{
    if (!b) return F2Q_EINVAL;
    if (n_reads) *n_reads = b->n_reads;
    if (n_general) *n_general = b->n_general;
    if (device_bytes) *device_bytes = b->dev_bytes;
    return F2Q_OK;
}

// host-packed tiles and raw records -> a resident block of n_reads reads (or pairs)
static int block_from_packed(f2q_ctx *c, const HostPacked &hp, uint64_t n_reads, f2q_block **out)
{
    f2q_block *b = new f2q_block();
    b->n_reads = n_reads; b->n_general = hp.g_len.size();
    int rc = F2Q_OK;
    do {
        if (hp.n_tiles) {
            uint32_t *db, *dq; uint16_t *dl;
            if ((rc = dev_upload(c, hp.bases.data(), hp.bases.size(), &db, b->allocs))) break;
            if ((rc = dev_upload(c, hp.qual.data(), hp.qual.size(), &dq, b->allocs))) break;
            if ((rc = dev_upload(c, hp.len.data(), hp.len.size(), &dl, b->allocs))) break;
            uint32_t *dci = nullptr;
            if (c->prm.mode == 1 && (rc = dev_upload(c, hp.c_index.data(), hp.c_index.size(), &dci, b->allocs))) break;
            b->pb.index = dci;
            b->pb.n_slots = (uint64_t)hp.n_tiles * F2Q_TILE; b->pb.n_tiles = hp.n_tiles;
            b->pb.wb = hp.wb; b->pb.wq = hp.wq; b->pb.rmax = hp.rmax; b->pb.planar_nw = hp.planar_nw;
            b->pb.bases = db; b->pb.qual = dq; b->pb.len = dl;
            b->dev_bytes += hp.bases.size() * 4 + hp.qual.size() * 4 + hp.len.size() * 2;
        }
        if (!hp.g_len.empty()) {
            uint8_t *dr; unsigned long long *doff; uint32_t *dlen, *dqlen, *dix;
            if ((rc = dev_upload(c, hp.raw.data(), hp.raw.size(), &dr, b->allocs))) break;
            if ((rc = dev_upload(c, hp.g_off.data(), hp.g_off.size(), &doff, b->allocs))) break;
            if ((rc = dev_upload(c, hp.g_len.data(), hp.g_len.size(), &dlen, b->allocs))) break;
            if ((rc = dev_upload(c, hp.g_qlen.data(), hp.g_qlen.size(), &dqlen, b->allocs))) break;
            if ((rc = dev_upload(c, hp.g_index.data(), hp.g_index.size(), &dix, b->allocs))) break;
            b->rb.n = hp.g_len.size(); b->rb.raw = dr; b->rb.off = doff; b->rb.len = dlen; b->rb.qlen = dqlen; b->rb.index = dix;
            if (!hp.g_len1.empty()) {                    // merged pairs
                uint32_t *dl1, *dq1;
                if ((rc = dev_upload(c, hp.g_len1.data(), hp.g_len1.size(), &dl1, b->allocs))) break;
                if ((rc = dev_upload(c, hp.g_qlen1.data(), hp.g_qlen1.size(), &dq1, b->allocs))) break;
                b->rb.len1 = dl1; b->rb.qlen1 = dq1;
            }
            if (!hp.hdr_umi.empty()) {                   // a header-UMI context: one entry per record of the block
                unsigned long long *dh;
                if ((rc = dev_upload(c, hp.hdr_umi.data(), hp.hdr_umi.size(), &dh, b->allocs))) break;
                b->rb.hdr_umi = dh;
                b->dev_bytes += hp.hdr_umi.size() * 8;
            }
            b->dev_bytes += hp.raw.size() + hp.g_len.size() * 20;
            b->raw_key_bytes = hp.raw.size();
        }
        hipError_t e = hipStreamSynchronize(c->stream);      // host staging vectors die with this frame
        if (e != hipSuccess) { rc = fail(c, F2Q_EHIP, hipGetErrorString(e)); break; }
    } while (0);
    if (rc) { free_all(c, b->allocs); delete b; return rc; }
    *out = b;
    return F2Q_OK;
}

static int block_from_records(f2q_ctx *c, const std::vector<Rec> &recs, f2q_block **out)
{
    HostPacked hp;
    pack_records(c->plan, recs, hp);
    if (c->umi.hdr_sep) header_umis(recs, recs.size(), (uint32_t)c->umi.hdr_sep, (uint32_t)c->umi.dev.length, hp.hdr_umi);
    return block_from_packed(c, hp, recs.size(), out);
}


// out[i] = in[0] + ... + in[i-1] on the context's stream (k_scan_blocks / k_scan_sums / k_scan_add)
static int exclusive_scan(f2q_ctx *c, const uint32_t *in, uint32_t *out, uint32_t n, std::vector<void *> &tmp)
{
    if (!n) return F2Q_OK;
    const uint32_t n_blocks = (n + F2Q_SCAN_BLOCK - 1u) / F2Q_SCAN_BLOCK;
    uint32_t *sums;
    int rc = dev_alloc(c, (size_t)n_blocks, &sums, tmp);
    if (rc) return rc;
    hipLaunchKernelGGL(k_scan_blocks, dim3(n_blocks), dim3(F2Q_SCAN_THREADS), 0, c->stream, in, out, n, sums);
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(F2Q_SCAN_THREADS), 0, c->stream, sums, n_blocks);
    hipLaunchKernelGGL(k_scan_add, dim3(n_blocks), dim3(F2Q_SCAN_THREADS), 0, c->stream, out, n, sums);
    HIPC(c, hipGetLastError());
    return F2Q_OK;
}

// FASTQ text -> resident block, framing and packing done by the device (k_nl_count .. k_pack).  Handles up to
// 2 GiB of text per call; *consumed = bytes up to the end of the last complete record.
// text that is already (on its way) in device memory: `buf` is the allocation (it becomes the block's), `text` the
// 16-byte aligned start of the FASTQ bytes inside it, with room for the census padding behind them
struct DevText { void *buf = nullptr; size_t cap = 0; uint8_t *text = nullptr; uint8_t last_byte = 0; bool borrowed = false; };   // borrowed: the caller keeps the allocation (f2q_text)

// One text on the device, framed: its line starts (k_nl_count -> scan -> k_line_starts).  The text is copied from `fastq`
// into an allocation pushed to `text_owner`, or is already (on its way) in device memory (`pre`).  ft.sentinel is the source of
// an asynchronous 4-byte copy: ft must outlive the next wait on the stream.
struct FramedText { uint8_t *text = nullptr; uint32_t *ls = nullptr; uint32_t n_chunks = 0, n_newlines = 0, sentinel = 0; uint64_t n_lines = 0; };
static int frame_text_device(f2q_ctx *c, const uint8_t *fastq, size_t nbytes, const DevText *pre, std::vector<void *> &text_owner,
                             std::vector<void *> &tmp, FramedText &ft)
{
    int rc;
    ft.n_chunks = (uint32_t)((nbytes + F2Q_NL_CHUNK - 1) / F2Q_NL_CHUNK);
    const uint32_t n_chunks = ft.n_chunks;
    const size_t padded = (size_t)n_chunks * F2Q_NL_CHUNK + 16;
    uint32_t *d_cc, *d_cp;
    if (pre) {
        ft.text = pre->text;
        if ((size_t)(ft.text - (uint8_t *)pre->buf) + padded > pre->cap) return fail(c, F2Q_EINVAL, "staged text buffer too small");
    } else if ((rc = dev_alloc(c, padded, &ft.text, text_owner))) return rc;
    if ((rc = dev_alloc(c, (size_t)n_chunks + 1, &d_cc, tmp, 0))) return rc;
    if ((rc = dev_alloc(c, (size_t)n_chunks + 1, &d_cp, tmp))) return rc;
    HIPC(c, hipMemsetAsync(ft.text + nbytes, 0, padded - nbytes, c->stream));
    const double tc0 = now_ms();
    if (!pre) HIPC(c, hipMemcpyAsync(ft.text, fastq, nbytes, hipMemcpyHostToDevice, c->stream));
    if (c->trace) { HIPC(c, hipStreamSynchronize(c->stream)); c->tr_copy += now_ms() - tc0; }
    hipLaunchKernelGGL(k_nl_count, dim3(n_chunks), dim3(256), 0, c->stream, ft.text, (uint64_t)nbytes, d_cc);
    HIPC(c, hipGetLastError());
    if ((rc = exclusive_scan(c, d_cc, d_cp, (uint32_t)n_chunks + 1u, tmp))) return rc;
    HIPC(c, hipMemcpyAsync(&ft.n_newlines, d_cp + n_chunks, 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    const bool open_tail = nbytes > 0 && (pre ? pre->last_byte : fastq[nbytes - 1]) != '\n';
    ft.n_lines = (uint64_t)ft.n_newlines + (open_tail ? 1 : 0);
    if ((rc = dev_alloc(c, (size_t)ft.n_newlines + 2, &ft.ls, tmp))) return rc;
    hipLaunchKernelGGL(k_line_starts, dim3(n_chunks), dim3(256), 0, c->stream, ft.text, (uint64_t)nbytes, d_cp, ft.ls);
    HIPC(c, hipGetLastError());
    ft.sentinel = (uint32_t)nbytes + 1u;
    HIPC(c, hipMemcpyAsync(ft.ls + ft.n_newlines + 1, &ft.sentinel, 4, hipMemcpyHostToDevice, c->stream));
    return F2Q_OK;
}

// *cons = bytes of a framed text up to the end of its record n_rec - 1: the start of line 4 * n_rec, or everything when
// that record's last line is unterminated.  Queued on the stream: *cons holds it after the next wait.
static int consumed_offset(f2q_ctx *c, const FramedText &ft, size_t nbytes, uint32_t n_rec, uint32_t *cons)
{
    *cons = (uint32_t)nbytes;
    if ((uint64_t)4 * n_rec <= ft.n_newlines) HIPC(c, hipMemcpyAsync(cons, ft.ls + (size_t)4 * n_rec, 4, hipMemcpyDeviceToHost, c->stream));
    return F2Q_OK;
}

// The compact tiles of a block's n_clean clean reads, rmax_in the longest of their packed lengths: the planes are
// allocated into `own`, described in b->pb and handed to the packing kernel in o (PackOut or PairPackOut).
template <class Out>
static int alloc_tile_planes(f2q_ctx *c, f2q_block *b, std::vector<void *> &own, uint32_t n_clean, uint32_t rmax_in, Out &o)
{
    if (!n_clean) return F2Q_OK;
    int rc;
    uint32_t rmax, nw, wb, wq;
    tile_geometry(c->plan, rmax_in, rmax, nw, wb, wq);
    const uint32_t n_tiles = (n_clean + F2Q_TILE - 1) / F2Q_TILE;
    if ((rc = dev_alloc(c, (size_t)n_tiles * wb * F2Q_TILE, &o.bases, own, 0))) return rc;
    if ((rc = dev_alloc(c, (size_t)n_tiles * wq * F2Q_TILE, &o.qual, own, 0))) return rc;
    if ((rc = dev_alloc(c, (size_t)n_tiles * F2Q_TILE, &o.len, own, 0xFF))) return rc;
    if (c->prm.mode == 1 && (rc = dev_alloc(c, (size_t)n_tiles * F2Q_TILE, &o.c_index, own, 0))) return rc;
    o.wb = wb; o.wq = wq;
    b->pb.n_slots = (uint64_t)n_tiles * F2Q_TILE; b->pb.n_tiles = n_tiles; b->pb.wb = wb; b->pb.wq = wq; b->pb.rmax = rmax;
    b->pb.planar_nw = nw; b->pb.bases = o.bases; b->pb.qual = o.qual; b->pb.len = o.len; b->pb.index = o.c_index;
    b->dev_bytes += (uint64_t)n_tiles * F2Q_TILE * ((wb + wq) * 4 + 2);
    return F2Q_OK;
}

// ---- the UMI in the read header (f2q_set_umi_header) ----------------------------------------------------------------
// The array a header-UMI context's raw records take their UMI from (RawBlock::hdr_umi): one entry per record of the text,
// written by k_header_umi on the stream, owned by the block (`own`).  Nothing is launched on any other context.
static int header_umis_device(f2q_ctx *c, const FramedText &ft, uint32_t n_rec, std::vector<void *> &own, unsigned long long **out)
{
    *out = nullptr;
    if (!c->umi.hdr_sep) return F2Q_OK;
    HeaderUmiDev d{};
    d.text = ft.text; d.line_start = ft.ls; d.n_records = n_rec; d.sep = (uint32_t)c->umi.hdr_sep; d.length = (uint32_t)c->umi.dev.length;
    if (int rc = dev_alloc(c, (size_t)n_rec, &d.out, own)) return rc;
    hipLaunchKernelGGL(k_header_umi, dim3((n_rec + F2Q_ING_THREADS - 1u) / F2Q_ING_THREADS), dim3(F2Q_ING_THREADS), 0, c->stream, d);
    HIPC(c, hipGetLastError());
    EC_POINT(c, "k_header_umi");
    *out = d.out;
    return F2Q_OK;
}
// F2Q_TRACE=1: HIP-event times of the ingest kernels of one text (k_classify, k_header_umi, k_pack), printed once the block
// is made; without it nothing is created or recorded
struct IngestTrace {
    f2q_ctx *c; hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    explicit IngestTrace(f2q_ctx *ctx) : c(ctx) { if (c->trace) for (hipEvent_t &e : ev) if (hipEventCreate(&e) != hipSuccess) e = nullptr; }
    ~IngestTrace() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    void mark(int i) { if (ev[i]) (void)hipEventRecord(ev[i], c->stream); }
    void print(uint32_t n_rec, bool header)             // after the stream has been waited for
    {
        if (!ev[0]) return;
        float ms[3] = {0, 0, 0};
        for (int k = 0; k < 3; k++) if (k != 1 || header) (void)hipEventElapsedTime(&ms[k], ev[2 * k], ev[2 * k + 1]);
        fprintf(stderr, "[f2q trace] ingest kernels: %u records, k_classify %.4f ms, k_header_umi %.4f ms, k_pack %.4f ms\n", n_rec, ms[0], ms[1], ms[2]);
    }
    IngestTrace(const IngestTrace &) = delete;
};

// Both device ingest drivers keep their scratch in `tmp` and what the block will own in `own` until they hand the block
// out: any return before that waits for the stream and frees both.
static int block_from_text_device(f2q_ctx *c, const uint8_t *fastq, size_t nbytes, size_t *consumed, f2q_block **out,
                                  const DevText *pre = nullptr, uint64_t max_records = ~0ull)
{
    *out = nullptr; *consumed = 0;
    FramedText ft;                                   // (outlives the scopes' wait for the stream: ft.sentinel)
    std::unique_ptr<f2q_block> b(new f2q_block());
    DevScope tmp(c), own(c);
    if (pre && !pre->borrowed) own.v.push_back(pre->buf);
    if (nbytes == 0) { *out = b.release(); return F2Q_OK; }    // an empty buffer is an empty block
    int rc;
    if ((rc = frame_text_device(c, fastq, nbytes, pre, own.v, tmp.v, ft))) return rc;
    const uint32_t n_rec = (uint32_t)std::min<uint64_t>(ft.n_lines / 4, max_records);   // (a piece of a sharded file owns only the records that start in it)
    b->n_reads = n_rec;
    if (n_rec == 0) { HIPC(c, hipStreamSynchronize(c->stream)); b->allocs.swap(own.v); *out = b.release(); return F2Q_OK; }
    uint32_t cons32;
    if ((rc = consumed_offset(c, ft, nbytes, n_rec, &cons32))) return rc;
    IngestDev ing{};
    ing.text = ft.text; ing.line_start = ft.ls; ing.n_records = n_rec;
    uint32_t *d_before;
    for (uint32_t **p : {&ing.r_off, &ing.r_len, &ing.r_qoff, &ing.r_qlen})
        if ((rc = dev_alloc(c, (size_t)n_rec, p, tmp.v))) return rc;
    if ((rc = dev_alloc(c, (size_t)n_rec + 1, &ing.clean, tmp.v, 0))) return rc;
    if ((rc = dev_alloc(c, (size_t)n_rec + 1, &d_before, tmp.v))) return rc;
    if ((rc = dev_alloc(c, (size_t)4, &ing.meta, tmp.v, 0))) return rc;
    const unsigned igrid = (unsigned)((n_rec + F2Q_ING_THREADS - 1u) / F2Q_ING_THREADS);
    IngestTrace trace(c);
    trace.mark(0);
    hipLaunchKernelGGL(k_classify, dim3(igrid), dim3(F2Q_ING_THREADS), 0, c->stream, ing, c->plan);
    HIPC(c, hipGetLastError());
    trace.mark(1);
    unsigned long long *d_hdr;
    trace.mark(2);
    if ((rc = header_umis_device(c, ft, n_rec, own.v, &d_hdr))) return rc;
    trace.mark(3);
    if ((rc = exclusive_scan(c, ing.clean, d_before, n_rec + 1u, tmp.v))) return rc;
    uint32_t n_clean = 0, rmax_in = 0;
    HIPC(c, hipMemcpyAsync(&n_clean, d_before + n_rec, 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(&rmax_in, ing.meta, 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    *consumed = cons32;
    const uint32_t n_dirty = n_rec - n_clean;
    PackOut o{};
    if ((rc = alloc_tile_planes(c, b.get(), own.v, n_clean, rmax_in, o))) return rc;
    o.planar_nw = b->pb.planar_nw;
    if (n_dirty) {
        if ((rc = dev_alloc(c, (size_t)n_dirty, &o.g_off, own.v))) return rc;
        if ((rc = dev_alloc(c, (size_t)n_dirty, &o.g_qoff, own.v))) return rc;
        for (uint32_t **p : {&o.g_len, &o.g_qlen, &o.g_index})
            if ((rc = dev_alloc(c, (size_t)n_dirty, p, own.v))) return rc;
        b->rb.n = n_dirty; b->rb.raw = ft.text; b->rb.off = o.g_off; b->rb.qoff = o.g_qoff; b->rb.len = o.g_len;
        b->rb.qlen = o.g_qlen; b->rb.index = o.g_index; b->rb.hdr_umi = d_hdr;
        b->dev_bytes += nbytes + (d_hdr ? (uint64_t)n_rec * 8 : 0);
        b->raw_key_bytes = nbytes;                    // the records point into the text: no key is longer than its record
    }
    b->n_general = n_dirty;
    trace.mark(4);
    hipLaunchKernelGGL(k_pack, dim3(igrid), dim3(F2Q_ING_THREADS), 0, c->stream, ing, c->plan, d_before, o);
    HIPC(c, hipGetLastError());
    trace.mark(5);
    HIPC(c, hipStreamSynchronize(c->stream));         // scratch dies with this frame
    trace.print(n_rec, d_hdr != nullptr);
    b->allocs.swap(own.v); *out = b.release();
    return F2Q_OK;
}

extern "C" int f2q_block_from_fastq(f2q_ctx *c, const uint8_t *fastq, size_t nbytes, f2q_block **out)
{
    if (!c || !out || (!fastq && nbytes)) return F2Q_EINVAL;
    if (int rc = single_only(c)) return rc;
    HIPC(c, hipSetDevice(c->device));
    if (!c->host_pack && nbytes < ((size_t)1 << 31)) { size_t used; return block_from_text_device(c, fastq, nbytes, &used, out); }
    std::vector<Rec> recs;
    frame_fastq(fastq, nbytes, recs);
    return block_from_records(c, recs, out);
}

// one window of text (at most 1 GiB: the device packer indexes it with 32 bits): frame, pack, count, free
static int count_window(f2q_ctx *c, const uint8_t *fastq, size_t take, const DevText *pre, size_t *used_out, f2q_timing *one,
                        uint64_t max_records = ~0ull)
{
    f2q_block *b = nullptr; size_t used = 0;
    int rc;
    const double t0 = now_ms();
    if (!c->host_pack || pre || max_records != ~0ull) rc = block_from_text_device(c, fastq, take, &used, &b, pre, max_records);
    else {
        std::vector<Rec> recs;
        used = frame_fastq(fastq, take, recs);
        rc = recs.empty() ? F2Q_OK : block_from_records(c, recs, &b);
    }
    if (rc) return rc;
    const double t1 = now_ms();
    if (b && b->n_reads) rc = launch_block(c, b, one);
    if (c->trace) (void)hipStreamSynchronize(c->stream);
    const double t2 = now_ms();
    if (b) f2q_block_free(c, b);
    c->tr_frame += t1 - t0; c->tr_count += t2 - t1; c->tr_free += now_ms() - t2;
    *used_out = used;
    return rc;
}

extern "C" int f2q_count_block(f2q_ctx *c, const uint8_t *fastq, size_t nbytes, size_t *consumed, f2q_timing *t)
{
    if (!c || (!fastq && nbytes)) return F2Q_EINVAL;
    if (int rc = single_only(c)) return rc;
    HIPC(c, hipSetDevice(c->device));
    if (t) { memset(t, 0, sizeof *t); HIPC(c, hipEventRecord(c->ev_a, c->stream)); }
    if (consumed) *consumed = 0;
    int rc = F2Q_OK;
    size_t pos = 0;
    f2q_timing sum; memset(&sum, 0, sizeof sum);
    while (pos < nbytes) {
        // the device packer indexes the text with 32 bits: feed it at most 1 GiB at a time (record aligned by itself)
        const size_t take = std::min<size_t>(nbytes - pos, (size_t)1 << 30);
        size_t used = 0;
        f2q_timing one; memset(&one, 0, sizeof one);
        rc = count_window(c, fastq + pos, take, nullptr, &used, t ? &one : nullptr);
        if (rc) return rc;
        timing_add(sum, one);
        if (used == 0) break;                          // no complete record left in this window
        pos += used;
        if (take < ((size_t)1 << 30)) break;           // that was the tail: what is left is a partial record
    }
    if (consumed) *consumed = pos;
    return timing_close(c, t, sum);
}

// ---- paired-end samples: feature parts taken from both mates -------------------------------------------------------
extern "C" int f2q_set_mate2(f2q_ctx *c, const int32_t *start2, int32_t n_start2, int32_t revcomp)
{
    if (!c) return F2Q_EINVAL;
    if (c->have_lib || c->n_mate1) return fail(c, F2Q_ESTATE, "f2q_set_mate2 comes once, after f2q_create and before f2q_set_features");
    if (int rc = raw_mode_no_mate2(c)) return rc;
    if (!c->run_h.fixed) return fail(c, F2Q_EINVAL, "paired-end runs take fixed windows only (--st): anchored mates are not implemented");
    if (!start2 || n_start2 < 1 || c->prm.n_start + n_start2 > F2Q_MAX_ITER) return fail(c, F2Q_EINVAL, "mate 2 needs 1 .. 16 - n_start windows");
    for (int i = 0; i < n_start2; i++) if (start2[i] < 0) return fail(c, F2Q_EINVAL, "a mate-2 window starts before the mate");
    const f2q_params keep = c->prm;
    HIPC(c, hipSetDevice(c->device));
    c->n_mate1 = c->prm.n_start; c->rc2 = revcomp != 0;
    for (int i = 0; i < n_start2; i++) c->prm.start[c->prm.n_start + i] = start2[i];
    c->prm.n_start += n_start2;
    int rc = setup_run(c);
    if (rc) { c->prm = keep; c->n_mate1 = 0; c->rc2 = false; (void)setup_run(c); return rc; }
    HIPC(c, hipMemcpyAsync(c->run_d, &c->run_h, sizeof(RunDev), hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return F2Q_OK;
}

// Two FASTQ texts (each below 1 GiB: 32-bit offsets) -> a resident block of min(records1, records2) pairs; framing and
// packing done by the device (k_nl_count .. k_pack_paired).  *used1 / *used2 = bytes up to the end of the last record used.
static int block_from_pairs_device(f2q_ctx *c, const uint8_t *fq1, size_t n1, const uint8_t *fq2, size_t n2, size_t *used1, size_t *used2,
                                   f2q_block **out)
{
    *out = nullptr; *used1 = *used2 = 0;
    FramedText t1, t2;
    std::unique_ptr<f2q_block> b(new f2q_block());
    if (n1 == 0 || n2 == 0) { *out = b.release(); return F2Q_OK; }
    DevScope tmp(c), own(c);                         // (the texts are scratch too: raw records are copies)
    int rc;
    if ((rc = frame_text_device(c, fq1, n1, nullptr, tmp.v, tmp.v, t1))) return rc;
    if ((rc = frame_text_device(c, fq2, n2, nullptr, tmp.v, tmp.v, t2))) return rc;
    const uint32_t n_rec = (uint32_t)std::min<uint64_t>(t1.n_lines / 4, t2.n_lines / 4);
    b->n_reads = n_rec;
    if (n_rec == 0) { HIPC(c, hipStreamSynchronize(c->stream)); *out = b.release(); return F2Q_OK; }
    uint32_t cons1, cons2;
    if ((rc = consumed_offset(c, t1, n1, n_rec, &cons1))) return rc;
    if ((rc = consumed_offset(c, t2, n2, n_rec, &cons2))) return rc;
    PairIngestDev ing{};
    ing.text1 = t1.text; ing.text2 = t2.text; ing.ls1 = t1.ls; ing.ls2 = t2.ls; ing.n_pairs = n_rec;
    uint32_t *d_before, *d_raw_before;
    for (uint32_t **p : {&ing.off1, &ing.len1, &ing.qoff1, &ing.qlen1, &ing.off2, &ing.len2, &ing.qoff2, &ing.qlen2})
        if ((rc = dev_alloc(c, (size_t)n_rec, p, tmp.v))) return rc;
    if ((rc = dev_alloc(c, (size_t)n_rec + 1, &ing.clean, tmp.v, 0))) return rc;
    if ((rc = dev_alloc(c, (size_t)n_rec + 1, &ing.raw_bytes, tmp.v, 0))) return rc;
    if ((rc = dev_alloc(c, (size_t)n_rec + 1, &d_before, tmp.v))) return rc;
    if ((rc = dev_alloc(c, (size_t)n_rec + 1, &d_raw_before, tmp.v))) return rc;
    if ((rc = dev_alloc(c, (size_t)4, &ing.meta, tmp.v, 0))) return rc;
    const unsigned igrid = (unsigned)((n_rec + F2Q_ING_THREADS - 1u) / F2Q_ING_THREADS);
    hipLaunchKernelGGL(k_classify_paired, dim3(igrid), dim3(F2Q_ING_THREADS), 0, c->stream, ing, c->plan);
    HIPC(c, hipGetLastError());
    unsigned long long *d_hdr;                       // the UMI of a pair is the one in mate 1's header
    if ((rc = header_umis_device(c, t1, n_rec, own.v, &d_hdr))) return rc;
    if ((rc = exclusive_scan(c, ing.clean, d_before, n_rec + 1u, tmp.v))) return rc;
    if ((rc = exclusive_scan(c, ing.raw_bytes, d_raw_before, n_rec + 1u, tmp.v))) return rc;
    // 32-bit sizes with EVERY pair raw (a paired UMI context): a merged record holds only bytes of its four lines, each text
    // is below 1 GiB, so raw_total and every prefix of raw_bytes stay below 2^30 + 2^30 = 2^31 < 2^32; n_rec < 2^28 (a record has 4 newlines)
    uint32_t n_clean = 0, rmax_in = 0, raw_total = 0;
    HIPC(c, hipMemcpyAsync(&n_clean, d_before + n_rec, 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(&raw_total, d_raw_before + n_rec, 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(&rmax_in, ing.meta, 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    *used1 = cons1; *used2 = cons2;
    const uint32_t n_dirty = n_rec - n_clean;
    PairPackOut o{};
    if ((rc = alloc_tile_planes(c, b.get(), own.v, n_clean, rmax_in, o))) return rc;
    if (n_dirty) {
        if ((rc = dev_alloc(c, (size_t)raw_total + 16, &o.raw, own.v, 0))) return rc;
        if ((rc = dev_alloc(c, (size_t)n_dirty, &o.g_off, own.v))) return rc;
        for (uint32_t **p : {&o.g_len, &o.g_qlen, &o.g_len1, &o.g_qlen1, &o.g_index})
            if ((rc = dev_alloc(c, (size_t)n_dirty, p, own.v))) return rc;
        b->rb.n = n_dirty; b->rb.raw = o.raw; b->rb.off = o.g_off; b->rb.len = o.g_len; b->rb.qlen = o.g_qlen;
        b->rb.len1 = o.g_len1; b->rb.qlen1 = o.g_qlen1; b->rb.index = o.g_index; b->rb.hdr_umi = d_hdr;
        b->dev_bytes += (uint64_t)raw_total + (uint64_t)n_dirty * 28 + (d_hdr ? (uint64_t)n_rec * 8 : 0);
        b->raw_key_bytes = raw_total;                // no key is longer than its merged record
    }
    b->n_general = n_dirty;
    hipLaunchKernelGGL(k_pack_paired, dim3(igrid), dim3(F2Q_ING_THREADS), 0, c->stream, ing, c->plan, d_before, d_raw_before, o);
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(c->stream));         // scratch dies with this frame
    b->allocs.swap(own.v); *out = b.release();
    return F2Q_OK;
}

// steps over up to k newlines of buf[pos, n): how many it saw, and the offset behind the last of them (n when the text
// ends before the k-th)
struct LineStep { size_t pos; uint64_t seen; };
static LineStep skip_lines(const uint8_t *buf, size_t n, size_t pos, uint64_t k)
{
    uint64_t seen = 0;
    while (seen < k && pos < n) {
        const uint8_t *nl = (const uint8_t *)memchr(buf + pos, '\n', n - pos);
        if (!nl) { pos = n; break; }
        pos = (size_t)(nl - buf) + 1; seen++;
    }
    return LineStep{pos, seen};
}

// a window of each text (each below 1 GiB) -> a block of pairs; the host twin under F2Q_HOST_PACK=1
static int pair_block(f2q_ctx *c, const uint8_t *fq1, size_t n1, const uint8_t *fq2, size_t n2, size_t *used1, size_t *used2, f2q_block **out)
{
    if (!c->host_pack) return block_from_pairs_device(c, fq1, n1, fq2, n2, used1, used2, out);
    std::vector<Rec> r1, r2;
    frame_fastq(fq1, n1, r1); frame_fastq(fq2, n2, r2);
    const size_t n = std::min(r1.size(), r2.size());
    r1.resize(n); r2.resize(n);
    *used1 = skip_lines(fq1, n1, 0, 4 * (uint64_t)n).pos; *used2 = skip_lines(fq2, n2, 0, 4 * (uint64_t)n).pos;
    HostPacked hp;
    pack_pairs(c->plan, r1, r2, hp);
    if (c->umi.hdr_sep) header_umis(r1, n, (uint32_t)c->umi.hdr_sep, (uint32_t)c->umi.dev.length, hp.hdr_umi);
    return block_from_packed(c, hp, n, out);
}

static const size_t F2Q_PAIR_WINDOW = (size_t)1 << 30;      // most text of one mate per block (32-bit offsets on the device)

extern "C" int f2q_block_from_fastq_paired(f2q_ctx *c, const uint8_t *fastq1, size_t n1, const uint8_t *fastq2, size_t n2, f2q_block **out)
{
    if (!c || !out || (!fastq1 && n1) || (!fastq2 && n2)) return F2Q_EINVAL;
    if (int rc = paired_only(c)) return rc;
    if (n1 >= F2Q_PAIR_WINDOW || n2 >= F2Q_PAIR_WINDOW) return fail(c, F2Q_EINVAL, "a resident block of pairs holds less than 1 GiB of text per mate");
    HIPC(c, hipSetDevice(c->device));
    size_t u1, u2;
    return pair_block(c, fastq1, n1, fastq2, n2, &u1, &u2, out);
}

extern "C" int f2q_count_block_paired(f2q_ctx *c, const uint8_t *fastq1, size_t n1, const uint8_t *fastq2, size_t n2,
                                      size_t *consumed1, size_t *consumed2, f2q_timing *t)
{
    if (!c || (!fastq1 && n1) || (!fastq2 && n2)) return F2Q_EINVAL;
    if (int rc = paired_only(c)) return rc;
    HIPC(c, hipSetDevice(c->device));
    if (t) { memset(t, 0, sizeof *t); HIPC(c, hipEventRecord(c->ev_a, c->stream)); }
    if (consumed1) *consumed1 = 0;
    if (consumed2) *consumed2 = 0;
    size_t p1 = 0, p2 = 0;
    f2q_timing sum; memset(&sum, 0, sizeof sum);
    while (p1 < n1 && p2 < n2) {
        const size_t take1 = std::min(n1 - p1, F2Q_PAIR_WINDOW - 1), take2 = std::min(n2 - p2, F2Q_PAIR_WINDOW - 1);
        // a window that is not the text's tail ends with a whole line: an open last line would count as a line
        size_t w1 = take1, w2 = take2;
        if (p1 + w1 < n1) while (w1 > 0 && fastq1[p1 + w1 - 1] != '\n') w1--;
        if (p2 + w2 < n2) while (w2 > 0 && fastq2[p2 + w2 - 1] != '\n') w2--;
        f2q_block *b = nullptr; size_t u1 = 0, u2 = 0;
        int rc = pair_block(c, fastq1 + p1, w1, fastq2 + p2, w2, &u1, &u2, &b);
        if (rc) return rc;
        f2q_timing one; memset(&one, 0, sizeof one);
        if (b && b->n_reads) rc = launch_block(c, b, t ? &one : nullptr);
        const bool none = !b || b->n_reads == 0;
        if (b) f2q_block_free(c, b);
        if (rc) return rc;
        timing_add(sum, one);
        if (none) break;                               // no complete pair left in these windows
        p1 += u1; p2 += u2;
        if (p1 + (w1 - u1) >= n1 && p2 + (w2 - u2) >= n2) break;     // both windows reached their text's end
    }
    if (consumed1) *consumed1 = p1;
    if (consumed2) *consumed2 = p2;
    return timing_close(c, t, sum);
}

// ---- FASTQ text resident in device memory ------------------------------------------------------------------
struct f2q_text { void *buf = nullptr; size_t cap = 0, nbytes = 0; uint8_t last = 0; };

extern "C" int f2q_text_upload(f2q_ctx *c, const uint8_t *fastq, size_t nbytes, f2q_text **out)
{
    if (!c || !out || (!fastq && nbytes)) return F2Q_EINVAL;
    if (nbytes > ((size_t)1 << 30)) return fail(c, F2Q_EINVAL, "f2q_text_upload: at most 1 GiB of text (the device framing indexes a text with 32 bits)");
    HIPC(c, hipSetDevice(c->device));
    f2q_text *t = new f2q_text();
    const size_t n_chunks = (nbytes + F2Q_NL_CHUNK - 1) / F2Q_NL_CHUNK;
    t->cap = n_chunks * F2Q_NL_CHUNK + 16; t->nbytes = nbytes; t->last = nbytes ? fastq[nbytes - 1] : 0;
    hipError_t e = hipMalloc(&t->buf, t->cap);
    if (e == hipSuccess && nbytes) e = hipMemcpyAsync(t->buf, fastq, nbytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { if (t->buf) (void)hipFree(t->buf); delete t; return fail(c, F2Q_EHIP, std::string("f2q_text_upload: ") + hipGetErrorString(e)); }
    *out = t;
    return F2Q_OK;
}

extern "C" int f2q_count_text(f2q_ctx *c, f2q_text *txt, size_t *consumed, f2q_timing *t)
{
    if (!c || !txt) return F2Q_EINVAL;
    if (int rc = single_only(c)) return rc;
    HIPC(c, hipSetDevice(c->device));
    if (t) { memset(t, 0, sizeof *t); HIPC(c, hipEventRecord(c->ev_a, c->stream)); }
    if (consumed) *consumed = 0;
    DevText pre; pre.buf = txt->buf; pre.cap = txt->cap; pre.text = (uint8_t *)txt->buf; pre.last_byte = txt->last; pre.borrowed = true;
    size_t used = 0;
    f2q_timing one; memset(&one, 0, sizeof one);
    int rc = txt->nbytes ? count_window(c, nullptr, txt->nbytes, &pre, &used, t ? &one : nullptr) : F2Q_OK;
    if (rc) return rc;
    if (consumed) *consumed = used;
    return timing_close(c, t, one);
}

extern "C" void f2q_text_free(f2q_ctx *c, f2q_text *t)
{
    if (!t) return;
    if (c) { (void)hipSetDevice(c->device); if (c->stream) (void)hipStreamSynchronize(c->stream); }
    if (t->buf) (void)hipFree(t->buf);
    delete t;
}

extern "C" int f2q_text_read(f2q_ctx *c, const f2q_text *t, uint8_t *dst, size_t cap, size_t *nbytes)
{
    if (!c || !t || !nbytes) return F2Q_EINVAL;
    *nbytes = t->nbytes;
    if (!dst) return F2Q_OK;
    if (cap < t->nbytes) return fail(c, F2Q_EINVAL, "f2q_text_read: the buffer is smaller than the text");
    HIPC(c, hipSetDevice(c->device));
    if (t->nbytes) HIPC(c, hipMemcpyAsync(dst, t->buf, t->nbytes, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return F2Q_OK;
}

// ---- BGZF members inflated on the device (k_inflate_bgzf) ----------------------------------------------------------
// the member table of n members whose compressed bytes lie in d_in (in_cap bytes, table included if it is there):
// inflate into d_text (text_cap bytes) on c->stream and bring the n result words back.  The first member whose status
// is not OK is *first_bad (n: none).
static int inflate_members(f2q_ctx *c, const uint8_t *d_in, uint64_t in_cap, const BgzfMember *d_mem, uint32_t n, uint8_t *d_text,
                           uint64_t text_cap, std::vector<BgzfResult> &res, uint32_t *first_bad)
{
    res.assign(n, BgzfResult{});
    *first_bad = n;
    if (n == 0) return F2Q_OK;
    DevScope tmp(c);
    BgzfResult *d_res;
    int rc = dev_alloc(c, n, &d_res, tmp.v, 0xFF);
    if (rc) return rc;
    // LDS holds two workgroups per CU; each walks its share of the members
    const uint32_t grid = std::min<uint32_t>(n, (uint32_t)c->n_cu * 2u);
    hipLaunchKernelGGL(k_inflate_bgzf, dim3(grid), dim3(64), 0, c->stream, d_in, in_cap, d_mem, n, d_text, text_cap, d_res);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(res.data(), d_res, (size_t)n * sizeof(BgzfResult), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, F2Q_EHIP, std::string("k_inflate_bgzf: ") + hipGetErrorString(e));
    for (uint32_t i = 0; i < n; i++) if (res[i].status != F2Q_INF_OK) { *first_bad = i; break; }
    return F2Q_OK;
}

// offset of the first byte after the last '\n' of members [0, n) (0: none), and the last byte of their text
static void members_tail(const std::vector<BgzfMember> &ms, const std::vector<BgzfResult> &res, uint32_t n, uint64_t &cut, int &last_byte)
{
    cut = 0; last_byte = -1;
    for (uint32_t i = n; i-- > 0;) {
        if (last_byte < 0 && ms[i].isize) last_byte = (int)res[i].last_byte;
        if (res[i].last_nl) { cut = ms[i].out_off + res[i].last_nl; break; }
    }
    for (uint32_t i = n; last_byte < 0 && i-- > 0;) if (ms[i].isize) last_byte = (int)res[i].last_byte;
}

// The table entry of the BGZF member at p (avail bytes from there on): its deflate bytes start at in_base + header, its
// text goes to out_off; CRC and ISIZE come from its trailer.  -1: no whole member there; 0: damaged, the block size has
// no room for header and trailer; 1: m and bsize are set.
static int bgzf_entry(const uint8_t *p, size_t avail, uint64_t in_base, uint64_t out_off, BgzfMember &m, uint32_t &bsize)
{
    uint32_t hdr;
    if (!TextSource::bgzf_member(p, avail, bsize, hdr) || bsize > avail) return -1;
    if (bsize < hdr + 8) return 0;
    const uint8_t *t = p + bsize - 8;
    m = BgzfMember{};
    m.in_off = in_base + hdr; m.in_len = bsize - hdr - 8; m.out_off = (uint32_t)out_off;
    m.crc = t[0] | (t[1] << 8) | (t[2] << 16) | ((uint32_t)t[3] << 24);
    m.isize = t[4] | (t[5] << 8) | (t[6] << 16) | ((uint32_t)t[7] << 24);
    return 1;
}

// The member index of a BGZF file (compressed offsets, text sizes) cut into runs of whole members: a new run starts
// when the member would take the run's text past text_cap or, with a byte_cap, its compressed bytes and member table
// past byte_cap.  A run of empty members keeps its place.
struct MemberRun { size_t m0, m1; uint64_t text, bytes; };
static std::vector<MemberRun> member_runs(const std::vector<uint64_t> &off, const std::vector<uint32_t> &isz, uint64_t file_size,
                                          uint64_t text_cap, uint64_t byte_cap = 0)
{
    std::vector<MemberRun> runs;
    for (size_t i = 0; i < off.size(); i++) {
        const uint64_t bs = (i + 1 < off.size() ? off[i + 1] : file_size) - off[i];
        if (runs.empty() || runs.back().text + isz[i] > text_cap ||
            (byte_cap && runs.back().bytes + bs + sizeof(BgzfMember) * (runs.back().m1 - runs.back().m0 + 1) + 16 > byte_cap))
            runs.push_back(MemberRun{i, i, 0, 0});
        MemberRun &r = runs.back();
        r.m1 = i + 1; r.text += isz[i]; r.bytes += bs;
    }
    return runs;
}

extern "C" int f2q_text_from_bgzf(f2q_ctx *c, const uint8_t *bgzf, size_t nbytes, f2q_text **out)
{
    if (!c || !out || (!bgzf && nbytes)) return F2Q_EINVAL;
    *out = nullptr;
    // the member table (a damaged header ends it: the members before it are what the text holds)
    std::vector<BgzfMember> ms;
    uint64_t text = 0;
    bool bad = false;
    for (size_t pos = 0; pos < nbytes;) {
        uint32_t bsize; BgzfMember m;
        const int got = bgzf_entry(bgzf + pos, nbytes - pos, pos, text, m, bsize);
        if (got < 0) return fail(c, F2Q_EUNSUPPORTED, "f2q_text_from_bgzf: the buffer is not a run of whole BGZF members");
        if (got == 0) { bad = true; break; }
        if (m.isize > F2Q_INF_OUT_BYTES) return fail(c, F2Q_EUNSUPPORTED, "f2q_text_from_bgzf: a member holds more than 64 KiB of text");
        text += m.isize;
        if (text > ((uint64_t)1 << 30)) return fail(c, F2Q_EINVAL, "f2q_text_from_bgzf: at most 1 GiB of text (the device framing indexes a text with 32 bits)");
        ms.push_back(m);
        pos += bsize;
    }
    HIPC(c, hipSetDevice(c->device));
    std::vector<void *> tmp;
    uint8_t *d_in; BgzfMember *d_mem;
    int rc = dev_alloc(c, nbytes + 64, &d_in, tmp);
    if (!rc) rc = dev_upload(c, ms.data(), ms.size(), &d_mem, tmp);
    if (!rc && nbytes) rc = hip_rc(c, hipMemcpyAsync(d_in, bgzf, nbytes, hipMemcpyHostToDevice, c->stream));
    f2q_text *t = new f2q_text();
    const size_t n_chunks = ((size_t)text + F2Q_NL_CHUNK - 1) / F2Q_NL_CHUNK;
    t->cap = n_chunks * F2Q_NL_CHUNK + 16;
    if (!rc) { hipError_t e = hipMalloc(&t->buf, t->cap); if (e != hipSuccess) rc = fail(c, F2Q_EHIP, std::string("hipMalloc: ") + hipGetErrorString(e)); }
    std::vector<BgzfResult> res;
    uint32_t fb = 0;
    if (!rc) rc = inflate_members(c, d_in, nbytes + 64, d_mem, (uint32_t)ms.size(), (uint8_t *)t->buf, text, res, &fb);
    free_all(c, tmp);
    if (rc) { if (t->buf) (void)hipFree(t->buf); delete t; return rc; }
    t->nbytes = fb < ms.size() ? ms[fb].out_off : text;
    uint64_t cut; int lb;
    members_tail(ms, res, fb, cut, lb);
    t->last = lb < 0 ? 0 : (uint8_t)lb;
    *out = t;
    if (bad || fb < ms.size()) return fail(c, F2Q_ETRUNCATED, "f2q_text_from_bgzf: a damaged member; the text ends before it");
    return F2Q_OK;
}

// ---- file streaming -------------------------------------------------------------------------------
// Page-locked staging buffers are expensive to create (tens of ms per 256 MiB) and every file needs two, so
// they are kept in a small process-wide pool between files (and between contexts: --cp runs several at once).
struct PinBuf { uint8_t *p = nullptr; size_t cap = 0; bool pageable = false; };
struct PinnedPool {
    std::mutex mu;
    std::vector<PinBuf> idle;
    size_t idle_bytes = 0;
    static constexpr size_t KEEP_BYTES = (size_t)1600 << 20;
    bool acquire(size_t cap, PinBuf &out)
    {
        {
            std::lock_guard<std::mutex> g(mu);
            size_t best = idle.size();
            for (size_t i = 0; i < idle.size(); i++)
                if (idle[i].cap >= cap && (best == idle.size() || idle[i].cap < idle[best].cap)) best = i;
            if (best < idle.size()) { out = idle[best]; idle_bytes -= out.cap; idle.erase(idle.begin() + (ptrdiff_t)best); return true; }
        }
        out.p = nullptr; out.cap = cap; out.pageable = false;
        if (hipHostMalloc((void **)&out.p, cap, hipHostMallocPortable) == hipSuccess) return true;
        (void)hipGetLastError();                          // no page-locked memory to be had: ordinary memory works too,
        out.pageable = true;                              // the copies to the device are just staged by the runtime
        out.p = (uint8_t *)malloc(cap);
        return out.p != nullptr;
    }
    void release(PinBuf &b)
    {
        if (!b.p) return;
        {
            std::lock_guard<std::mutex> g(mu);
            if (!b.pageable && idle_bytes + b.cap <= KEEP_BYTES && idle.size() < 8) { idle.push_back(b); idle_bytes += b.cap; b = PinBuf(); return; }
        }
        if (b.pageable) free(b.p); else (void)hipHostFree(b.p);
        b = PinBuf();
    }
};
static PinnedPool g_pinned;

// One piece of text in a pinned slot, as the reader thread describes it: n bytes at the slot's head room, the text to
// count starting a bytes into them.  The last piece holds no text; it only ends the stream.
struct Piece { int slot = -1; size_t n = 0, a = 0; uint64_t max_records = ~0ull, first_read = 0; bool ok = true, last = false; };
// a piece's text copied ahead to the device, `head` bytes into the buffer
struct Staged { void *buf = nullptr; size_t cap = 0; int slot = -1; size_t n = 0; };

// free a staged copy once `s`, the last stream to touch it, is done with it
static void free_staged(f2q_ctx *c, Staged &st, hipStream_t s)
{
    if (!st.buf) return;
    (void)hipStreamSynchronize(s);
    { DevScope own(c, st.buf); }
    st = Staged();
}

// The piece pipeline of f2q_count_file(_shard) and f2q_count_pieces.  Three pinned slots: one being counted, one ready
// (its text possibly already travelling to the device), one being filled by the reader thread with fill(j, p, pc):
// piece j's text goes to p, `head` bytes into the slot, and pc describes it.  next() hands the pieces over in order.
// When staging is allowed, the text of the piece after the one handed over is copied to the device on c->copy_stream
// while that one is counted; next() makes c->stream wait for that copy and leaves it in `cur`.  The destructor stops
// and joins the reader and gives back every buffer, so no return path leaves a joinable thread or a held buffer
// behind; whatever fill uses must outlive the PieceStream.
struct PieceStream {
    static constexpr int NSLOT = 3;
    f2q_ctx *const c;
    size_t head = 0;
    bool can_stage = false, force_stage = false;
    PinBuf buf[NSLOT];
    std::mutex mu; std::condition_variable cv;
    std::deque<Piece> ready; bool slot_free[NSLOT] = {true, true, true}; bool stop = false;
    std::thread reader;
    Staged staged;                                 // the text of the next piece, on its way to the device
    Staged cur;                                    // the text of the piece next() handed over, if it was sent ahead
    double pin_ms = 0, read_ms = 0, wait_ms = 0;   // (F2Q_TRACE) getting the slots, the reader busy, next() waiting for it

    explicit PieceStream(f2q_ctx *ctx) : c(ctx) {}
    ~PieceStream() { close(); }
    uint8_t *text(const Piece &pc) const { return buf[pc.slot].p + head; }

    template <class Fill> int start(size_t head_room, size_t slot_bytes, bool stage, Fill fill)
    {
        head = head_room; can_stage = stage; force_stage = getenv("F2Q_FORCE_STAGING") != nullptr;
        const double p0 = now_ms();
        for (auto &b : buf) if (!g_pinned.acquire(slot_bytes, b)) return fail(c, F2Q_ENOMEM, "cannot allocate the read buffers");
        pin_ms = now_ms() - p0;
        if (can_stage && !c->copy_stream) {
            hipError_t e = hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_copy, hipEventDisableTiming);
            if (e != hipSuccess) return fail(c, F2Q_EHIP, std::string("copy stream: ") + hipGetErrorString(e));
        }
        reader = std::thread([this, fill]() {
            for (uint64_t j = 0;; j++) {
                const int slot = (int)(j % NSLOT);
                { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return slot_free[slot] || stop; }); if (stop) return; slot_free[slot] = false; }
                Piece pc; pc.slot = slot;
                const double r0 = now_ms();
                fill(j, buf[slot].p + head, pc);
                read_ms += now_ms() - r0;
                { std::lock_guard<std::mutex> g(mu); ready.push_back(pc); }
                cv.notify_all();
                if (pc.last) return;
            }
        });
        return F2Q_OK;
    }

    Piece next()
    {
        Piece pc;
        { const double w0 = now_ms(); std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return !ready.empty(); }); pc = ready.front(); ready.pop_front(); wait_ms += now_ms() - w0; }
        if (staged.buf && staged.slot == pc.slot && staged.n == pc.n) {
            cur = staged; staged = Staged();
            if (hipStreamWaitEvent(c->stream, c->ev_copy, 0) != hipSuccess) { (void)hipGetLastError(); (void)hipStreamSynchronize(c->copy_stream); }
        } else free_staged(c, staged, c->copy_stream);
        if (!pc.last) stage_next();                // the piece after this one, if the reader has it already
        return pc;
    }

    // the caller is done with the piece (a staged copy it left in `cur` was not used); with stop_now no more are read
    void done(const Piece &pc, bool stop_now)
    {
        free_staged(c, cur, c->stream);
        { std::lock_guard<std::mutex> g(mu); slot_free[pc.slot] = true; if (stop_now) stop = true; }
        cv.notify_all();
    }

    void close()
    {
        free_staged(c, cur, c->stream);
        free_staged(c, staged, c->copy_stream);
        { std::lock_guard<std::mutex> g(mu); stop = true; }
        cv.notify_all();
        if (reader.joinable()) reader.join();
        for (auto &b : buf) g_pinned.release(b);
    }

  private:
    void stage_next()
    {
        if (!can_stage || staged.buf) return;
        Piece nx;
        {
            std::unique_lock<std::mutex> lk(mu);
            if (force_stage) cv.wait(lk, [&] { return !ready.empty(); });      // tests: every piece takes this path
            if (!ready.empty()) nx = ready.front();
        }
        if (nx.slot < 0 || nx.n == 0 || !nx.ok) return;
        const size_t cap = head + nx.n + 2 * (size_t)F2Q_NL_CHUNK + 64;
        if (dev_get(c, cap, &staged.buf) != F2Q_OK) { staged = Staged(); return; }   // no memory for it: the piece takes the ordinary path
        staged.cap = cap; staged.slot = nx.slot; staged.n = nx.n;
        if (hipMemcpyAsync((uint8_t *)staged.buf + head, buf[nx.slot].p + head, nx.n, hipMemcpyHostToDevice, c->copy_stream) != hipSuccess ||
            hipEventRecord(c->ev_copy, c->copy_stream) != hipSuccess) {
            (void)hipGetLastError();
            free_staged(c, staged, c->copy_stream);
        }
    }
};

// Count n bytes of text that are in device memory (or on their way there), `off` bytes into the buffer st; their last byte
// is last_byte.  The tail_n host bytes at `tail` (a carried tail) are first put on c->stream at the head of the text.  The
// up to 15 bytes between the 16-byte boundary below the text and the text are filled with 'x': they lengthen the first
// line, a record's header line, which is never looked at (fast2q.py:324-328 takes lines 2 and 4 only).  With `keep` the
// caller keeps the buffer; otherwise, unless the call fails before framing, it belongs to the block from here on and st
// is emptied.  *used counts from the start of the text.
static int count_dev_text(f2q_ctx *c, Staged &st, bool keep, size_t off, const uint8_t *tail, size_t tail_n, size_t n, uint8_t last_byte,
                          uint64_t max_records, size_t *used, f2q_timing *one)
{
    const size_t al = off & ~(size_t)15, lead = off - al;
    uint8_t *d = (uint8_t *)st.buf;
    if (tail_n) HIPC(c, hipMemcpyAsync(d + off, tail, tail_n, hipMemcpyHostToDevice, c->stream));
    if (lead) HIPC(c, hipMemsetAsync(d + al, 'x', lead, c->stream));
    DevText pre; pre.buf = st.buf; pre.cap = st.cap; pre.text = d + al; pre.last_byte = last_byte; pre.borrowed = keep;
    if (!keep) st = Staged();
    size_t used_dev = 0;
    const int rc = count_window(c, nullptr, lead + n, &pre, &used_dev, one, max_records);
    *used = used_dev > lead ? used_dev - lead : 0;
    return rc;
}

// reads_counter's file half (fast2q.py:560-578).  A reader thread (f2q_reader.h: parallel pread / parallel BGZF
// inflate / gzread) fills one pinned buffer while the device frames, packs and counts the other; whole lines only
// are handed over, the unconsumed tail (a partial record) is carried in front of the next piece.
// The framing of a piece that another rank counts: how many records it holds and where the last complete one ends
// (the same verdict block_from_text_device reaches on the device), from a newline census by the worker pool.
static size_t skip_piece(const uint8_t *p, size_t n, int threads, uint64_t *n_records)
{
    *n_records = 0;
    if (n == 0) return 0;
    const size_t slice_min = (size_t)1 << 20;
    const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)threads, n / slice_min));
    std::vector<uint64_t> cnt((size_t)T, 0);
    auto bounds = [&](int t, size_t &a, size_t &b) { a = n * (size_t)t / (size_t)T; b = n * (size_t)(t + 1) / (size_t)T; };
    auto work = [&](int t) {
        size_t a, b; bounds(t, a, b);
        uint64_t k = 0;
        for (size_t i = a; i < b; i++) k += (p[i] == 0x0a);
        cnt[(size_t)t] = k;
    };
    if (T == 1) work(0);
    else {
        std::vector<std::thread> th;
        for (int t = 1; t < T; t++) th.emplace_back(work, t);
        work(0);
        for (auto &x : th) x.join();
    }
    uint64_t n_nl = 0; for (uint64_t k : cnt) n_nl += k;
    const uint64_t n_lines = n_nl + (p[n - 1] != 0x0a ? 1 : 0);
    const uint64_t n_rec = n_lines / 4;
    *n_records = n_rec;
    if (n_rec == 0) return 0;
    if (4 * n_rec > n_nl) return n;                       // the last record's last line has no newline: everything
    // position after the (4 * n_rec)-th newline
    uint64_t want = 4 * n_rec, seen = 0;
    for (int t = 0; t < T; t++) {
        if (seen + cnt[(size_t)t] >= want) {
            size_t a, b; bounds(t, a, b);
            for (size_t i = a; i < b; i++) if (p[i] == 0x0a && ++seen == want) return i + 1;
        }
        seen += cnt[(size_t)t];
    }
    return n;
}

// f2q_count_file on a BGZF file with F2Q_DEVICE_INFLATE=1 (count_file_impl decides).  Pieces are runs of whole members
// with at most CH bytes of text, as piece_map cuts them; the reader thread only preads each run's compressed bytes into
// a pinned slot behind its member table, and PieceStream sends both to the device ahead.  k_inflate_bgzf writes the
// text behind the head room of a device text buffer; the carried tail (the partial record piece k leaves over) is
// copied device to device in front of it, the head room growing for a tail longer than 64 KiB.  The members before the
// first damaged one are counted, whole lines only, and nothing after it (read_bgzf's verdict).
static int count_bgzf_device(f2q_ctx *c, const char *path, TextSource &src, const std::vector<uint64_t> &off, const std::vector<uint32_t> &isz,
                             size_t CH, f2q_timing *t)
{
    const size_t HEAD = 64 << 10, MAX_WINDOW = (size_t)1 << 30;
    CH = std::min<size_t>(CH, (size_t)512 << 20);
    // the pieces: text <= CH, member table + compressed bytes <= PB (a run of empty members takes little text)
    const size_t PB = std::max<size_t>(CH, (size_t)1 << 20);
    const std::vector<MemberRun> runs = member_runs(off, isz, src.file_size, CH, PB);
    // what the reader leaves for each slot: the member table (also at the head of the slot) and a damaged header
    struct SlotInfo { std::vector<BgzfMember> ms; uint64_t text = 0; bool bad = false, io = false; };
    SlotInfo info[PieceStream::NSLOT];
    auto fill = [&](uint64_t j, uint8_t *p, Piece &pc) {
        if (j >= runs.size()) { pc.last = true; return; }
        const MemberRun &r = runs[j];
        SlotInfo &si = info[pc.slot];
        si = SlotInfo();
        const size_t nm = r.m1 - r.m0, T = (nm * sizeof(BgzfMember) + 15) & ~(size_t)15;
        uint8_t *z = p + T;
        // the run's compressed bytes, in slices of at least 4 MiB read by up to F2Q_IO_THREADS threads
        const int nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)src.n_threads, r.bytes / ((size_t)4 << 20)));
        std::atomic<bool> short_read{false};
        auto slice = [&](int k) {
            const size_t a = r.bytes * (size_t)k / (size_t)nt, b = r.bytes * (size_t)(k + 1) / (size_t)nt;
            for (size_t o = a; o < b;) { ssize_t g = pread(src.fd, z + o, b - o, (off_t)(off[r.m0] + o)); if (g <= 0) { short_read = true; return; } o += (size_t)g; }
        };
        std::vector<std::thread> th;
        for (int k = 1; k < nt; k++) th.emplace_back(slice, k);
        slice(0);
        for (auto &x : th) x.join();
        if (short_read) { si.io = true; pc.n = 0; return; }
        for (size_t i = r.m0; i < r.m1; i++) {
            const size_t at = (size_t)(off[i] - off[r.m0]);
            const uint32_t want = (uint32_t)((i + 1 < off.size() ? off[i + 1] : src.file_size) - off[i]);
            uint32_t bsize = 0; BgzfMember m;
            if (bgzf_entry(z + at, r.bytes - at, T + at, si.text, m, bsize) != 1 || bsize != want) { si.bad = true; break; }
            m.isize = isz[i];                        // (what the runs were cut by)
            si.ms.push_back(m); si.text += m.isize;
        }
        if (!si.ms.empty()) memcpy(p, si.ms.data(), si.ms.size() * sizeof(BgzfMember));
        pc.n = T + r.bytes;
    };
    PieceStream ps(c);
    int rc = ps.start(0, PB + 64, !getenv("F2Q_NO_STAGING"), fill);
    if (rc) return rc;
    f2q_timing sum; memset(&sum, 0, sizeof sum);
    double inflate_ms = 0;
    DevScope text(c);                               // owns the text buffer of the last piece ...
    Staged prev;                                    // ... this one; its tail [carry_at, carry_at + carry_n) is carried
    size_t carry_at = 0, carry_n = 0;
    uint8_t carry_last = 0;
    bool truncated = false;
    for (;;) {
        const Piece pc = ps.next();
        f2q_timing one; memset(&one, 0, sizeof one);
        if (pc.last) {                               // the last partial record, counted in place (:392)
            size_t used = 0;
            if (carry_n) rc = count_dev_text(c, prev, true, carry_at, nullptr, 0, carry_n, carry_last, ~0ull, &used, &one);
            timing_add(sum, one);
            ps.done(pc, true);
            break;
        }
        const SlotInfo &si = info[pc.slot];
        if (si.io) { rc = fail(c, F2Q_EIO, std::string("short read of ") + path); ps.done(pc, true); break; }
        const uint32_t nm = (uint32_t)si.ms.size();
        const size_t hr = std::max(HEAD, (carry_n + 15) & ~(size_t)15);
        const size_t cap = hr + (size_t)si.text + 2 * (size_t)F2Q_NL_CHUNK + 64;
        if (carry_n + si.text > MAX_WINDOW - (size_t)F2Q_NL_CHUNK) { rc = fail(c, F2Q_EINVAL, std::string(path) + ": a line longer than the device window"); ps.done(pc, true); break; }
        const double i0 = now_ms();
        void *tb = nullptr, *zb = nullptr;
        rc = dev_get(c, cap, &tb);
        std::vector<void *> scratch;
        const uint8_t *d_in = (const uint8_t *)ps.cur.buf;
        uint64_t in_cap = ps.cur.cap;
        if (!rc && !d_in) {                          // not sent ahead: copy it now
            rc = dev_get(c, pc.n + 64, &zb);
            if (!rc) { scratch.push_back(zb); d_in = (const uint8_t *)zb; in_cap = pc.n + 64; }
            if (!rc) rc = hip_rc(c, hipMemcpyAsync(zb, ps.text(pc), pc.n, hipMemcpyHostToDevice, c->stream));
        }
        if (!rc && carry_n) rc = hip_rc(c, hipMemcpyAsync((uint8_t *)tb + hr - carry_n, (uint8_t *)prev.buf + carry_at, carry_n, hipMemcpyDeviceToDevice, c->stream));
        std::vector<BgzfResult> res;
        uint32_t fb = nm;
        if (!rc) rc = inflate_members(c, d_in, in_cap, (const BgzfMember *)d_in, nm, (uint8_t *)tb + hr, si.text, res, &fb);
        free_all(c, scratch);
        inflate_ms += now_ms() - i0;
        free_all(c, text.v); prev = Staged();
        if (tb) { text.v.push_back(tb); prev.buf = tb; prev.cap = cap; }
        if (rc) { ps.done(pc, true); break; }
        const bool bad = si.bad || fb < nm;
        const uint64_t text_n = fb < nm ? si.ms[fb].out_off : si.text;
        uint64_t nl; int lb;
        members_tail(si.ms, res, fb, nl, lb);
        if (lb >= 0) carry_last = (uint8_t)lb;
        const size_t start = hr - carry_n, have = carry_n + (size_t)text_n;
        size_t used = 0;
        if (nl) {                                    // whole lines only: a line is never split between blocks
            // the framing zeroes the bytes behind the window: the partial line there is kept aside and put back
            const size_t cut = carry_n + (size_t)nl, rest = have - cut;
            DevScope own(c);
            uint8_t *aside = nullptr, *const rest_at = (uint8_t *)prev.buf + start + cut;
            if (rest) rc = dev_alloc(c, rest, &aside, own.v);
            if (!rc && rest) rc = hip_rc(c, hipMemcpyAsync(aside, rest_at, rest, hipMemcpyDeviceToDevice, c->stream));
            if (!rc) rc = count_dev_text(c, prev, true, start, nullptr, 0, cut, 0x0a, ~0ull, &used, &one);
            if (!rc && rest) rc = hip_rc(c, hipMemcpyAsync(rest_at, aside, rest, hipMemcpyDeviceToDevice, c->stream));
            timing_add(sum, one);
        }
        carry_at = start + used; carry_n = have - used;
        if (bad) truncated = true;
        ps.done(pc, rc || bad);
        if (rc || bad) break;
    }
    ps.close();
    if (t) *t = sum;
    if (c->trace) fprintf(stderr, "[f2q trace] %s (bgzf-device, %d io threads): pinned %.1f ms, reader busy %.1f ms, waited for reader %.1f ms, inflate %.1f ms, frame+pack %.1f ms (H2D copy %.1f), count %.1f ms, free %.1f ms\n",
                          path, src.n_threads, ps.pin_ms, ps.read_ms, ps.wait_ms, inflate_ms, c->tr_frame, c->tr_copy, c->tr_count, c->tr_free);
    if (rc) return rc;
    if (truncated) return fail(c, F2Q_ETRUNCATED, std::string(path) + " is an incomplete or corrupted gzip file");
    return F2Q_OK;
}

static int count_file_impl(f2q_ctx *c, const char *path, uint32_t rank, uint32_t world, f2q_timing *t)
{
    if (!c || !path || world == 0 || rank >= world) return F2Q_EINVAL;
    if (int rc = single_only(c)) return rc;
    if (int rc = raw_mode_one_rank(c, world)) return rc;
    HIPC(c, hipSetDevice(c->device));
    size_t CH = file_chunk_bytes((size_t)256 << 20);
    TextSource src;
    { std::string err; if (src.open(path, err) != 0) return fail(c, F2Q_EIO, err); }
    const size_t HEAD = 64 << 10;                  // room in front of each piece for the carried tail
    if (src.kind == TextSource::PLAIN && src.regular) CH = std::min<size_t>(CH, std::max<size_t>(src.file_size, 4096));
    else if (src.regular) CH = std::min<size_t>(CH, std::max<size_t>(src.file_size * 16, (size_t)4 << 20));
    // F2Q_DEVICE_INFLATE=1: a BGZF file of members of at most 64 KiB of text each is inflated on the device
    const char *dinf = getenv("F2Q_DEVICE_INFLATE");
    if (dinf && dinf[0] == '1' && world == 1 && !getenv("F2Q_HOST_PACK") && src.kind == TextSource::BGZF && src.regular) {
        std::vector<uint64_t> off; std::vector<uint32_t> isz;
        if (src.bgzf_index(off, isz) && std::all_of(isz.begin(), isz.end(), [](uint32_t s) { return s <= F2Q_INF_OUT_BYTES; }))
            return count_bgzf_device(c, path, src, off, isz, CH, t);
    }
    // The text of piece k+1 is copied to the device while piece k is framed, packed and counted.  Its carried tail is
    // only known once piece k is framed, so the piece lands HEAD bytes into its device buffer and the tail is put in
    // front of it later (count_dev_text).
    PieceStream ps(c);
    int rc = ps.start(HEAD, HEAD + CH, world == 1 && !c->host_pack && !getenv("F2Q_NO_STAGING"),
                      [&](uint64_t, uint8_t *p, Piece &pc) { pc.n = src.read(p, CH); pc.last = pc.n == 0; });
    if (rc) return rc;
    f2q_timing sum; memset(&sum, 0, sizeof sum);
    std::vector<uint8_t> carry, big;
    uint32_t piece_no = 0;                         // pieces are dealt to the ranks round robin
    for (;;) {
        const Piece pc = ps.next();
        const bool eof = pc.last;
        uint8_t *base; size_t have;
        if (carry.size() <= HEAD) {
            base = ps.text(pc) - carry.size();
            if (!carry.empty()) memcpy(base, carry.data(), carry.size());
            have = carry.size() + pc.n;
        } else {                                   // a tail longer than the head room (very long lines): pageable detour
            big.resize(carry.size() + pc.n);
            memcpy(big.data(), carry.data(), carry.size());
            if (pc.n) memcpy(big.data() + carry.size(), ps.text(pc), pc.n);
            base = big.data(); have = big.size();
        }
        size_t used = 0;
        if (have) {
            f2q_timing one; memset(&one, 0, sizeof one);
            size_t cut = have;                     // only whole lines: a line is never split between blocks
            // (at the end of a damaged archive too: readline raised there instead of returning the cut-off line, :405-407)
            if (!eof || src.truncated()) while (cut > 0 && base[cut - 1] != 0x0a) cut--;
            if (cut) {
                if (ps.cur.buf && carry.size() <= HEAD)
                    rc = count_dev_text(c, ps.cur, false, HEAD - carry.size(), carry.data(), carry.size(), cut, base[cut - 1], ~0ull, &used, &one);
                else if (piece_no % world == rank) rc = f2q_count_block(c, base, cut, &used, &one);
                else {                             // another rank's piece: only its framing matters here
                    uint64_t n_rec = 0;
                    used = skip_piece(base, cut, src.n_threads, &n_rec);
                    c->reads_seen += n_rec;
                }
                piece_no++;
            }
            if (eof) used = have;                  // trailing partial record is dropped (:392)
            timing_add(sum, one);
        }
        if (!rc) { std::vector<uint8_t> rest(base + used, base + have); carry.swap(rest); }
        ps.done(pc, rc || eof);
        if (rc || eof) break;
    }
    ps.close();
    if (t) *t = sum;
    if (c->trace) fprintf(stderr, "[f2q trace] %s (%s, %d io threads): pinned %.1f ms, reader busy %.1f ms, waited for reader %.1f ms, frame+pack %.1f ms (H2D copy %.1f), count %.1f ms, free %.1f ms\n",
                          path, src.kind_name(), src.n_threads, ps.pin_ms, ps.read_ms, ps.wait_ms, c->tr_frame, c->tr_copy, c->tr_count, c->tr_free);
    if (rc) return rc;
    if (src.truncated()) return fail(c, F2Q_ETRUNCATED, std::string(path) + " is an incomplete or corrupted gzip file");
    return F2Q_OK;
}

extern "C" int f2q_count_file(f2q_ctx *c, const char *path, f2q_timing *t) { return count_file_impl(c, path, 0, 1, t); }

// one process per GPU on the same file: every rank streams the whole file (the framing is global), counts the
// pieces k with k % world == rank on its device and only takes a newline census of the others
extern "C" int f2q_count_file_shard(f2q_ctx *c, const char *path, uint32_t rank, uint32_t world, f2q_timing *t)
{
    return count_file_impl(c, path, rank, world, t);
}

// ---- a paired-end sample by path: two files streamed in lockstep ----------------------------------------------------
// One piece of each file per round (F2Q_FILE_CHUNK bytes of text; a file whose carried tail already holds a piece's worth
// waits for the other), cut at whole lines, counted with the paired block call; what a round did not use is carried to
// the next.  The reads are synchronous and the buffers pageable: no thread, no pinned memory to give back on any return.
struct MateStream {
    TextSource src; std::vector<uint8_t> buf; size_t at = 0; bool eof = false;      // buf[at ..): text not used yet
    const uint8_t *data() const { return buf.data() + at; }
    size_t size() const { return buf.size() - at; }
    void fill(size_t chunk)
    {
        if (at) { buf.erase(buf.begin(), buf.begin() + (ptrdiff_t)at); at = 0; }    // once per read, not once per round
        const size_t have = buf.size();
        buf.resize(have + chunk);
        const size_t got = src.read(buf.data() + have, chunk);
        buf.resize(have + got);
        if (got == 0) eof = true;
    }
    // the bytes a block may see: whole lines only, except at the sound end of the data (a damaged archive's cut-off last
    // line is never seen, as readline raises there instead of returning it, fast2q.py:405-407)
    size_t whole() const
    {
        size_t cut = size();
        if (!eof || src.truncated()) while (cut > 0 && data()[cut - 1] != 0x0a) cut--;
        return cut;
    }
    // does it hold a complete record?  four lines, the last one possibly open at the sound end of the data
    bool has_record() const
    {
        const size_t n = whole();
        const LineStep s = skip_lines(data(), n, 0, 3);
        return s.seen == 3 && s.pos < n;
    }
};

extern "C" int f2q_count_file_paired(f2q_ctx *c, const char *path1, const char *path2, f2q_timing *t)
{
    if (!c || !path1 || !path2) return F2Q_EINVAL;
    if (int rc = paired_only(c)) return rc;
    HIPC(c, hipSetDevice(c->device));
    const size_t CH = std::min(file_chunk_bytes((size_t)64 << 20), F2Q_PAIR_WINDOW / 4);      // per piece and file
    MateStream m[2];
    { std::string err; if (m[0].src.open(path1, err) != 0) return fail(c, F2Q_EIO, err); }
    { std::string err; if (m[1].src.open(path2, err) != 0) return fail(c, F2Q_EIO, err); }
    if (c->trace) fprintf(stderr, "[f2q trace] paired: %s (%s) + %s (%s), pieces of %zu bytes\n", path1, m[0].src.kind_name(), path2, m[1].src.kind_name(), CH);
    f2q_timing sum; memset(&sum, 0, sizeof sum);
    int rc = F2Q_OK;
    bool stuck = false;                            // the last round used nothing: both files read on whatever they carry
    for (;;) {
        for (int k = 0; k < 2; k++) if (!m[k].eof && (stuck || m[k].size() < CH)) m[k].fill(CH);
        size_t used[2] = {0, 0};
        const size_t w0 = m[0].whole(), w1 = m[1].whole();
        if (w0 && w1) {
            f2q_timing one; memset(&one, 0, sizeof one);
            if ((rc = f2q_count_block_paired(c, m[0].data(), w0, m[1].data(), w1, &used[0], &used[1], &one))) break;
            timing_add(sum, one);
        }
        for (int k = 0; k < 2; k++) m[k].at += used[k];
        stuck = used[0] == 0 && used[1] == 0;
        // done when one file has ended and holds no further record: the other can complete no pair any more
        const bool end0 = m[0].eof && !m[0].has_record(), end1 = m[1].eof && !m[1].has_record();
        if (!end0 && !end1) continue;
        // does the other hold a complete record beyond the last pair?  (read on only as far as that takes)
        const int o = end0 ? 1 : 0;
        bool extra = !(end0 && end1) && m[o].has_record();
        while (!(end0 && end1) && !extra && !m[o].eof) { m[o].fill(CH); extra = m[o].has_record(); }
        if (t) *t = sum;
        for (int k = 0; k < 2; k++)
            if (m[k].src.truncated()) return fail(c, F2Q_ETRUNCATED, m[k].src.path + " is an incomplete or corrupted gzip file");
        if (extra) return fail(c, F2Q_EPAIRING, std::string(end0 ? path2 : path1) + " holds records beyond the last record of its mate file");
        return F2Q_OK;
    }
    if (t) *t = sum;
    return rc;
}

// ---- one plain file counted by several processes without anybody reading foreign bytes ------------------------------
// The 4-line framing is global (fast2q.py:324-328: a record is lines 4i..4i+3 of the FILE), so a rank can only frame its
// share once it knows how many lines precede it.  The file is cut into pieces of piece_bytes, piece k belongs to rank
// k % world, and the work is split in two steps around ONE small all-reduce that the caller does (it owns the
// communicator): (1) every rank counts the newlines of ITS pieces (f2q_census_pieces), (2) with the summed census every
// rank knows the line index at which each of its pieces starts and counts the records whose first line STARTS in
// its pieces, reading on past the piece's end only to finish its last record (f2q_count_pieces).
struct PieceSpan { uint64_t base, size; };
// a piece and its 1 MiB look-ahead are framed in one window, and the device framing indexes a window with 32 bits
// (count_file_impl and f2q_count_block cap their windows at 1 GiB for the same reason)
static const uint64_t F2Q_MAX_PIECE_BYTES = ((uint64_t)1 << 30) - ((uint64_t)2 << 20);
static inline bool piece_bytes_ok(uint64_t piece_bytes) { return piece_bytes >= 4096 && piece_bytes <= F2Q_MAX_PIECE_BYTES; }
static inline PieceSpan piece_span(uint64_t file_size, uint64_t piece_bytes, uint64_t k)
{
    const uint64_t base = k * piece_bytes;
    return PieceSpan{base, base < file_size ? std::min<uint64_t>(piece_bytes, file_size - base) : 0};
}

// how a file is cut: plain files by byte ranges; BGZF files by runs of whole members whose text adds up to at most
// piece_bytes (a member is <= 64 KiB of text and carries its text size in its trailer, so the cut needs no inflating)
struct PieceMap {
    bool bgzf = false;
    uint64_t n = 0, max_text = 0;
    std::vector<uint64_t> c_off, text;                     // BGZF: compressed offset of the piece's first member, its text bytes
};
static int piece_map(TextSource &src, const char *path, uint64_t piece_bytes, PieceMap &pm)
{
    pm = PieceMap();
    if (src.kind == TextSource::PLAIN && src.regular) {
        pm.n = (src.file_size + piece_bytes - 1) / piece_bytes; pm.max_text = std::min<uint64_t>(piece_bytes, src.file_size);
        return F2Q_OK;
    }
    if (!(src.kind == TextSource::BGZF && src.regular)) return F2Q_EUNSUPPORTED;
    // (the three calls of a run ask for the same map: keep the last one)
    static std::mutex mu; static std::string last_key; static PieceMap last;
    struct stat sb; if (stat(path, &sb) != 0) return F2Q_EIO;
    const std::string key = std::string(path) + "|" + std::to_string((unsigned long long)sb.st_size) + "|" + std::to_string((long long)sb.st_mtime) +
                            "|" + std::to_string((unsigned long long)piece_bytes);
    { std::lock_guard<std::mutex> g(mu); if (key == last_key) { pm = last; return F2Q_OK; } }
    std::vector<uint64_t> off; std::vector<uint32_t> isz;
    if (!src.bgzf_index(off, isz)) return F2Q_EUNSUPPORTED;
    pm.bgzf = true;
    for (const MemberRun &r : member_runs(off, isz, src.file_size, piece_bytes)) {
        pm.c_off.push_back(off[r.m0]); pm.text.push_back(r.text);
        pm.max_text = std::max(pm.max_text, r.text);
    }
    pm.n = pm.c_off.size();
    { std::lock_guard<std::mutex> g(mu); last_key = key; last = pm; }
    return F2Q_OK;
}

extern "C" int f2q_file_pieces(const char *path, uint64_t piece_bytes, uint64_t *n_pieces, int *shardable)
{
    if (!path || !n_pieces || !shardable || !piece_bytes_ok(piece_bytes)) return F2Q_EINVAL;
    *n_pieces = 0; *shardable = 0;
    TextSource src; std::string err;
    if (src.open(path, err) != 0) { g_create_err = err; return F2Q_EIO; }
    PieceMap pm;
    if (piece_map(src, path, piece_bytes, pm) == F2Q_OK) { *shardable = pm.bgzf ? 2 : 1; *n_pieces = pm.n; }
    return F2Q_OK;
}

// census[2k] = newlines in piece k, census[2k+1] = 1 if its last byte is a newline; only this rank's pieces are written
extern "C" int f2q_census_pieces(const char *path, uint32_t rank, uint32_t world, uint64_t piece_bytes, uint64_t *census, uint64_t n_pieces)
{
    if (!path || !census || world == 0 || rank >= world || !piece_bytes_ok(piece_bytes)) return F2Q_EINVAL;
    TextSource src; std::string err;
    if (src.open(path, err) != 0) { g_create_err = err; return F2Q_EIO; }
    PieceMap pm;
    if (piece_map(src, path, piece_bytes, pm) != F2Q_OK || pm.n != n_pieces) { g_create_err = "not a plain or BGZF regular file (or the pieces changed)"; return F2Q_EUNSUPPORTED; }
    if (pm.bgzf) {
        // inflate this rank's runs of members (the reader's member-parallel decoder) and count
        std::vector<uint8_t> b((size_t)std::min<uint64_t>(std::max<uint64_t>(pm.max_text, 1 << 16), (uint64_t)64 << 20));
        for (uint64_t k = rank; k < n_pieces; k += world) {
            uint64_t left = pm.text[k], nl = 0; uint8_t lastb = 0;
            if (!src.seek_bgzf(pm.c_off[k])) { g_create_err = "seek"; return F2Q_EIO; }
            while (left) {
                const size_t n = src.read(b.data(), (size_t)std::min<uint64_t>(b.size(), left));
                if (n == 0) { g_create_err = "BGZF member damaged or cut off"; return F2Q_EIO; }
                for (size_t j = 0; j < n; j++) nl += (b[j] == 0x0a);
                lastb = b[n - 1]; left -= n;
            }
            census[2 * k] = nl; census[2 * k + 1] = (pm.text[k] && lastb == 0x0a) ? 1 : 0;
        }
        return F2Q_OK;
    }
    const int T = src.n_threads;
    const size_t SL = (size_t)4 << 20;                                  // bytes per pread
    std::vector<std::vector<uint8_t>> bufs((size_t)T);
    for (uint64_t k = rank; k < n_pieces; k += world) {
        const PieceSpan sp = piece_span(src.file_size, piece_bytes, k);
        if (sp.size == 0) { census[2 * k] = 0; census[2 * k + 1] = 0; continue; }
        const uint64_t n_sl = (sp.size + SL - 1) / SL;
        std::vector<uint64_t> cnt((size_t)T, 0);
        std::atomic<uint64_t> next{0};
        std::atomic<bool> bad{false};
        auto work = [&](int t) {
            std::vector<uint8_t> &b = bufs[(size_t)t];
            if (b.size() < SL) b.resize(SL);
            for (;;) {
                const uint64_t i = next.fetch_add(1);
                if (i >= n_sl) return;
                const uint64_t off = sp.base + i * SL, len = std::min<uint64_t>(SL, sp.base + sp.size - off);
                uint64_t o = 0;
                while (o < len) { ssize_t r = pread(src.fd, b.data() + o, len - o, (off_t)(off + o)); if (r <= 0) { bad = true; return; } o += (uint64_t)r; }
                uint64_t n = 0;
                for (uint64_t j = 0; j < len; j++) n += (b[j] == 0x0a);
                cnt[(size_t)t] += n;
            }
        };
        std::vector<std::thread> th;
        for (int t = 1; t < T; t++) th.emplace_back(work, t);
        work(0);
        for (auto &x : th) x.join();
        if (bad) { g_create_err = "short read"; return F2Q_EIO; }
        uint64_t nl = 0; for (uint64_t v : cnt) nl += v;
        uint8_t lastb = 0;
        if (pread(src.fd, &lastb, 1, (off_t)(sp.base + sp.size - 1)) != 1) { g_create_err = "short read"; return F2Q_EIO; }
        census[2 * k] = nl; census[2 * k + 1] = lastb == 0x0a ? 1 : 0;
    }
    return F2Q_OK;
}

extern "C" int f2q_count_pieces(f2q_ctx *c, const char *path, uint32_t rank, uint32_t world, uint64_t piece_bytes,
                                const uint64_t *census, uint64_t n_pieces, f2q_timing *t)
{
    if (!c || !path || !census || world == 0 || rank >= world || !piece_bytes_ok(piece_bytes)) return F2Q_EINVAL;
    if (int rc = single_only(c)) return rc;
    if (int rc = raw_mode_one_rank(c, world)) return rc;
    HIPC(c, hipSetDevice(c->device));
    TextSource src;
    { std::string err; if (src.open(path, err) != 0) return fail(c, F2Q_EIO, err); }
    PieceMap pm;
    if (piece_map(src, path, piece_bytes, pm) != F2Q_OK) return fail(c, F2Q_EUNSUPPORTED, "f2q_count_pieces takes a plain or a BGZF regular file");
    if (n_pieces != pm.n) return fail(c, F2Q_EINVAL, "census does not fit the file");
    // what this rank owns: for every piece the text offset of its first record start, the number of records, the read index
    struct Job { uint64_t k, skip_lines, n_records, first_read; bool at_line_start; };
    std::vector<Job> jobs;
    {
        uint64_t lines_before = 0;                         // newlines before the piece = index of the line its first byte is in
        bool prev_ends_nl = true;                          // (the text before the piece ends with a newline, or there is none)
        for (uint64_t k = 0; k < n_pieces; k++) {
            const bool at_start = prev_ends_nl;
            const uint64_t nl = census[2 * k], last_nl = census[2 * k + 1];
            if (pm.bgzf ? pm.text[k] != 0 : piece_span(src.file_size, piece_bytes, k).size != 0) prev_ends_nl = last_nl != 0;
            else continue;                                 // an empty piece starts no line
            const uint64_t starts = (at_start ? 1 : 0) + nl - (last_nl ? 1 : 0);          // lines that START in the piece
            const uint64_t i0 = at_start ? lines_before : lines_before + 1;              // index of the first of them
            const uint64_t r0 = (i0 + 3) / 4 * 4;                                        // first record start at or after it
            if (k % world == rank && starts > r0 - i0) {
                const uint64_t left = starts - (r0 - i0);
                jobs.push_back(Job{k, r0 - i0, (left + 3) / 4, r0 / 4, at_start});
            }
            lines_before += nl;
        }
    }
    const size_t HEAD = 64, MARGIN = (size_t)1 << 20;       // a record that starts in the piece ends within the margin behind it
    PieceStream ps(c);
    const size_t slot_bytes = HEAD + (size_t)std::max<uint64_t>(pm.max_text, 4096) + MARGIN + (pm.bgzf ? (size_t)1 << 16 : 0);
    int rc = ps.start(HEAD, slot_bytes, !c->host_pack && !getenv("F2Q_NO_STAGING"), [&](uint64_t j, uint8_t *p, Piece &pc) {
        if (j == jobs.size()) { pc.last = true; return; }
        const Job &jb = jobs[j];
        PieceSpan sp = piece_span(src.file_size, piece_bytes, jb.k);
        uint64_t want = std::min<uint64_t>(sp.size + MARGIN, src.file_size - sp.base);
        size_t n = 0;
        if (!pm.bgzf) { n = src.read_at(sp.base, p, (size_t)want); pc.ok = n == want; }
        else {
            // the run of members, then members behind it until the last record is whole (4 newlines) or the margin is full
            sp.base = 0; sp.size = pm.text[jb.k];
            pc.ok = src.seek_bgzf(pm.c_off[jb.k]);
            while (pc.ok && n < sp.size) { const size_t g = src.read(p + n, (size_t)(sp.size - n)); if (!g) pc.ok = false; n += g; }
            size_t seen = 0, o = n;
            bool more = true;
            while (pc.ok && more && seen < 4 && n < sp.size + MARGIN) {
                const size_t g = src.read(p + n, (size_t)std::min<uint64_t>((uint64_t)1 << 16, sp.size + MARGIN - n));
                if (!g) { more = false; if (src.truncated()) pc.ok = false; break; }
                n += g;
                const LineStep s = skip_lines(p, n, o, 4 - seen);
                o = s.pos; seen += (size_t)s.seen;
            }
            // (for the check below: "the file goes on behind what was read" <=> the margin filled up without 4 newlines)
            want = n; sp.base = 0;
            const bool file_goes_on = more && seen < 4;
            if (file_goes_on) pc.ok = false;
        }
        // the first record start: the line after the one cut by the piece's start, then `skip_lines` more
        const size_t a = skip_lines(p, n, 0, jb.skip_lines + (jb.at_line_start ? 0 : 1)).pos;
        // the margin must hold the rest of the last record (4 more newlines, or the end of the file)
        if (!pm.bgzf && sp.base + want < src.file_size) {
            if (skip_lines(p, n, (size_t)sp.size, 4).seen < 4) pc.ok = false;           // lines too long for the margin: the caller falls back
        }
        pc.n = n; pc.a = a; pc.max_records = jb.n_records; pc.first_read = jb.first_read;
    });
    if (rc) return rc;
    f2q_timing sum; memset(&sum, 0, sizeof sum);
    for (;;) {
        const Piece pc = ps.next();
        if (!pc.ok) rc = fail(c, F2Q_EUNSUPPORTED, "a line longer than the piece margin (or a short read): count this file unsharded");
        if (!rc && !pc.last && pc.n > pc.a) {
            f2q_timing one; memset(&one, 0, sizeof one);
            size_t used = 0;
            c->reads_seen = pc.first_read;
            uint8_t *base = ps.text(pc) + pc.a;
            if (ps.cur.buf) rc = count_dev_text(c, ps.cur, false, HEAD + pc.a, nullptr, 0, pc.n - pc.a, base[pc.n - pc.a - 1], pc.max_records, &used, &one);
            else rc = count_window(c, base, pc.n - pc.a, nullptr, &used, &one, pc.max_records);
            timing_add(sum, one);
        }
        ps.done(pc, rc || pc.last);
        if (rc || pc.last) break;
    }
    if (t) *t = sum;
    return rc;
}

// ---- synthetic workload ---------------------------------------------------------------------------
extern "C" int f2q_synth_guides(f2q_ctx *c, const char *seqs, uint32_t n, uint32_t length)
{
    if (!c || !seqs || n == 0 || length < 1 || length > F2Q_REG_MAXLEN) return fail(c, F2Q_EINVAL, "f2q_synth_guides: bad argument");
    HIPC(c, hipSetDevice(c->device));
    std::vector<uint64_t> keys(n);
    for (uint32_t g = 0; g < n; g++)
        if (!feature_key((const uint8_t *)seqs + (size_t)g * length, length, keys[g])) return fail(c, F2Q_EINVAL, "synthetic guides must be ACGT");
    if (c->synth_keys_d) { (void)hipFree(c->synth_keys_d); c->synth_keys_d = nullptr; }
    HIPC(c, hipMalloc((void **)&c->synth_keys_d, (size_t)n * 8));
    HIPC(c, hipMemcpy(c->synth_keys_d, keys.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    c->synth_keys.swap(keys); c->synth_glen = length;
    return F2Q_OK;
}

static int synth_to_dev(f2q_ctx *c, const f2q_synth *s, SynthDev &d)
{
    memset(&d, 0, sizeof d);
    uint32_t glen;
    if (!c->synth_keys.empty()) { glen = c->synth_glen; d.n_guides = (int)c->synth_keys.size(); }
    else {
        if (!c->have_lib || c->ix.n_features == 0) return fail(c, F2Q_ESTATE, "synthetic reads need guides (f2q_set_features or f2q_synth_guides)");
        glen = c->ix.feat_off[1] - c->ix.feat_off[0];
        for (uint32_t f = 0; f < c->ix.n_features; f++) {
            uint64_t k;
            if (c->ix.feat_off[f + 1] - c->ix.feat_off[f] != glen || !feature_key(c->ix.feat_bytes.data() + c->ix.feat_off[f], glen, k))
                return fail(c, F2Q_EUNSUPPORTED, "synthetic reads need a uniform-length ACGT library (<= 31 bp)");
        }
        d.n_guides = (int)c->ix.n_features;
    }
    d.seed = s->seed; d.n_reads = s->n_reads; d.first_read = s->first_read;
    d.read_len = s->read_len; d.start = s->start; d.cassette = s->cassette; d.max_offset = s->max_offset;
    d.glen = (int)glen;
    d.t_sub = s->t_sub; d.t_rand = s->t_rand; d.t_n = s->t_n; d.t_lowq = s->t_lowq; d.t_q29 = s->t_q29; d.t_q28 = s->t_q28;
    if (s->read_len < 1 || s->read_len > F2Q_PACK_MAXLEN) return fail(c, F2Q_EINVAL, "read_len must be 1..512");
    if (s->cassette) {
        size_t ul = s->up ? strlen(s->up) : 0, dl = s->down ? strlen(s->down) : 0;
        if (ul > 63 || dl > 63) return fail(c, F2Q_EINVAL, "cassette flanks longer than 63");
        d.up_len = (int)ul; d.down_len = (int)dl;
        if (ul) memcpy(d.up, s->up, ul);
        if (dl) memcpy(d.down, s->down, dl);
    }
    return F2Q_OK;
}

extern "C" int f2q_synth_library(uint64_t seed, uint32_t n, uint32_t length, char *out)
{
    if (!out || length < 1 || length > 32) return F2Q_EINVAL;
    // tests/synth.py make_library: candidate k = bases of rnd(seed, k, 0); duplicates skipped
    std::vector<uint64_t> seen; seen.reserve(n);
    std::vector<uint64_t> sorted;
    uint64_t k = 0; uint32_t made = 0;
    const uint64_t mask = length >= 32 ? ~0ull : ((1ull << (2 * length)) - 1ull);
    // open-addressing set
    uint64_t cap = 16; while (cap < 4ull * n) cap <<= 1;
    std::vector<uint64_t> set(cap, ~0ull);
    std::vector<uint8_t> used(cap, 0);
    while (made < n) {
        uint64_t v = rnd(seed, k++, 0) & mask;
        uint64_t h = mix64(v) & (cap - 1);
        bool dup = false;
        while (used[h]) { if (set[h] == v) { dup = true; break; } h = (h + 1) & (cap - 1); }
        if (dup) continue;
        used[h] = 1; set[h] = v;
        for (uint32_t j = 0; j < length; j++) out[(size_t)made * length + j] = "ACGT"[(v >> (2 * j)) & 3];
        made++;
        if (k > 64ull * n + 1024) return F2Q_EINVAL;    // sequence space exhausted
    }
    return F2Q_OK;
}

extern "C" int f2q_synth_fastq(f2q_ctx *c, const f2q_synth *s, uint64_t lo, uint64_t hi, uint8_t *buf, size_t *nbytes)
{
    if (!c || !s || !nbytes || hi < lo) return F2Q_EINVAL;
    SynthDev d; int rc = synth_to_dev(c, s, d);
    if (rc) return rc;
    const int R = d.read_len;
    size_t need = 0;
    for (uint64_t i = lo; i < hi; i++) {
        char name[32]; int nl = snprintf(name, sizeof name, "@r%llu\n", (unsigned long long)i);
        need += (size_t)nl + (size_t)R + 3 + (size_t)R + 1;
    }
    if (!buf) { *nbytes = need; return F2Q_OK; }
    if (*nbytes < need) { *nbytes = need; return fail(c, F2Q_EINVAL, "buffer too small"); }
    size_t o = 0;
    const uint64_t *keys = c->synth_keys.empty() ? c->ix.key2.data() : c->synth_keys.data();
    for (uint64_t i = lo; i < hi; i++) {
        SynthRead r = synth_plan(d, i, [&](uint32_t g) { return keys[g]; });
        o += (size_t)snprintf((char *)buf + o, 32, "@r%llu\n", (unsigned long long)i);
        uint64_t fw = 0;
        for (int p = 0; p < R; p++) {
            if ((p & 31) == 0) fw = rnd(d.seed, i, F_FLANK0 + (p >> 5));
            buf[o + p] = synth_base(d, r, p, fw);
        }
        o += (size_t)R;
        buf[o++] = '\n'; buf[o++] = '+'; buf[o++] = '\n';
        for (int p = 0; p < R; p++) buf[o + p] = (p == r.qpos) ? r.qchar : (uint8_t)'I';
        o += (size_t)R;
        buf[o++] = '\n';
    }
    *nbytes = o;
    return F2Q_OK;
}

extern "C" int f2q_synth_create(f2q_ctx *c, const f2q_synth *s, f2q_block **out)
{
    if (!c || !s || !out) return F2Q_EINVAL;
    HIPC(c, hipSetDevice(c->device));
    if (int rc = single_only(c)) return rc;
    if (c->umi.hdr_sep) return fail(c, F2Q_ESTATE, "f2q_synth_create on a header-UMI context (f2q_set_umi_header): synthetic blocks have no headers");
    SynthDev d; int rc = synth_to_dev(c, s, d);
    if (rc) return rc;
    const int R = d.read_len;
    f2q_block *b = new f2q_block();
    b->n_reads = s->n_reads;
    const bool planar = c->plan.fast_anchor && R <= F2Q_ANCHOR_MAXLEN;
    const bool fast = c->plan.fast_fixed || planar;
    SynthOut o; memset(&o, 0, sizeof o);
    o.all_general = fast ? 0 : 1;
    o.inband_n = c->plan.inband_n ? 1 : 0;
    o.planar_nw = planar ? (R <= 96 ? 3u : R <= 160 ? 5u : 10u) : 0u;
    if (c->plan.fast_fixed && c->plan.n_win) {                     // several windows: the tiles hold the windows only
        o.n_win = c->plan.n_win; o.win_len = c->plan.win_len; o.win_end = c->plan.win_end;
        for (int i = 0; i < c->plan.n_win; i++) o.win_start[i] = c->plan.win_start[i];
    }
    const int Rs = o.n_win ? o.n_win * o.win_len : R;               // bases a tile stores per read
    const uint64_t n_tiles = (s->n_reads + F2Q_TILE - 1) / F2Q_TILE;
    const uint64_t n_slots = n_tiles * F2Q_TILE;
    // general-path capacity: everything, or the expected 'N' share with a wide margin
    double pn = (double)d.t_n / 4294967296.0;
    uint64_t gcap = fast ? (uint64_t)((double)s->n_reads * pn * 1.5 + 6.0 * sqrt((double)s->n_reads * pn + 1.0) + 1024.0) : s->n_reads;
    if (gcap > s->n_reads) gcap = s->n_reads;
    if (gcap == 0) gcap = 1;
    do {
        if (fast) {
            o.wb = planar ? 2 * o.planar_nw : (uint32_t)((Rs + 15) / 16);
            o.wq = planar ? 8 * o.planar_nw : (uint32_t)((Rs + 3) / 4);
            if ((rc = dev_alloc(c, (size_t)n_tiles * o.wb * F2Q_TILE, &o.bases, b->allocs, 0))) break;
            if ((rc = dev_alloc(c, (size_t)n_tiles * o.wq * F2Q_TILE, &o.qual, b->allocs, 0))) break;
            if ((rc = dev_alloc(c, (size_t)n_slots, &o.len, b->allocs))) break;
            b->dev_bytes += (uint64_t)n_tiles * (o.wb + o.wq) * F2Q_TILE * 4 + n_slots * 2;
        }
        if ((rc = dev_alloc(c, (size_t)gcap * 2 * R + 8, &o.raw, b->allocs))) break;
        if ((rc = dev_alloc(c, (size_t)gcap, &o.off, b->allocs))) break;
        if ((rc = dev_alloc(c, (size_t)gcap, &o.glen, b->allocs))) break;
        if ((rc = dev_alloc(c, (size_t)gcap, &o.gqlen, b->allocs))) break;
        if ((rc = dev_alloc(c, (size_t)gcap, &o.gindex, b->allocs))) break;
        if ((rc = dev_alloc(c, (size_t)1, &o.g_count, b->allocs, 0))) break;
        o.g_cap = gcap;
        hipLaunchKernelGGL(k_synth, dim3((unsigned)n_tiles), dim3(F2Q_TILE), 0, c->stream, d, c->synth_keys.empty() ? c->guide_keys_d : c->synth_keys_d, o, n_slots);
        hipError_t e = hipGetLastError();
        unsigned long long g = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&g, o.g_count, sizeof g, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { rc = fail(c, F2Q_EHIP, hipGetErrorString(e)); break; }
        if (g > gcap) { rc = fail(c, F2Q_ENOMEM, "synthetic general-path capacity exceeded"); break; }
        b->n_general = g;
        if (fast) {
            b->pb.n_slots = n_slots; b->pb.n_tiles = (uint32_t)n_tiles; b->pb.wb = o.wb; b->pb.wq = o.wq; b->pb.rmax = (uint32_t)Rs;
            b->pb.planar_nw = o.planar_nw;
            b->pb.bases = o.bases; b->pb.qual = o.qual; b->pb.len = o.len;
        }
        b->rb.n = g; b->rb.raw = o.raw; b->rb.off = o.off; b->rb.len = o.glen; b->rb.qlen = o.gqlen; b->rb.index = o.gindex;
        b->rb.first_index = 0;
        b->dev_bytes += g * (uint64_t)(2 * R + 20);
        b->raw_key_bytes = g * (uint64_t)R;
    } while (0);
    if (rc) { free_all(c, b->allocs); delete b; return rc; }
    *out = b;
    return F2Q_OK;
}

// ---- Extract+Count results ----------------------------------------------------------------------
// both Extract+Count tables, pulled to the host: the byte-string entries then the occupied single-word slots
struct EcHost {
    std::vector<std::string> keys;
    std::vector<unsigned long long> cnt, first;
};
static int ec_pull(f2q_ctx *c, EcHost &h)
{
    if (!c->ec.slots) return F2Q_OK;
    unsigned long long ctr[4];
    HIPC(c, hipMemcpyAsync(ctr, c->ec.ctr, sizeof ctr, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    if (ctr[2]) return fail(c, F2Q_ENOMEM, "Extract+Count table overflow (internal sizing error, code " + std::to_string(ctr[2]) + ")");
    const uint64_t n = ctr[0];
    if (n) {
        std::vector<uint32_t> len(n), arena(ctr[1] ? ctr[1] : 1);
        std::vector<unsigned long long> off(n), cnt(n), first(n);
        HIPC(c, hipMemcpy(len.data(), c->ec.ent_len, n * 4, hipMemcpyDeviceToHost));
        HIPC(c, hipMemcpy(off.data(), c->ec.ent_off, n * 8, hipMemcpyDeviceToHost));
        HIPC(c, hipMemcpy(cnt.data(), c->ec.ent_count, n * 8, hipMemcpyDeviceToHost));
        HIPC(c, hipMemcpy(first.data(), c->ec.ent_first, n * 8, hipMemcpyDeviceToHost));
        if (ctr[1]) HIPC(c, hipMemcpy(arena.data(), c->ec.arena, ctr[1] * 4, hipMemcpyDeviceToHost));
        for (uint64_t e = 0; e < n; e++) {
            if (off[e] + ((unsigned long long)len[e] + 3) / 4 > ctr[1])
                return fail(c, F2Q_ESTATE, "Extract+Count entry " + std::to_string(e) + " of " + std::to_string(n) + " is not filled in (offset " +
                            std::to_string(off[e]) + ", length " + std::to_string(len[e]) + ", arena " + std::to_string(ctr[1]) + " words)");
            h.keys.emplace_back((const char *)(arena.data() + off[e]), len[e]);
            h.cnt.push_back(cnt[e]); h.first.push_back(first[e]);
        }
    }
    if (ctr[3]) {
        const size_t ns = (size_t)c->ec.k64_mask + 1;
        std::vector<unsigned long long> ks(ns), kc(ns), kf(ns);
        HIPC(c, hipMemcpy(ks.data(), c->ec.k64_slots, ns * 8, hipMemcpyDeviceToHost));
        HIPC(c, hipMemcpy(kc.data(), c->ec.k64_count, ns * 8, hipMemcpyDeviceToHost));
        HIPC(c, hipMemcpy(kf.data(), c->ec.k64_first, ns * 8, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < ns; i++) {
            if (ks[i] == KEY_EMPTY) continue;
            char text[32];
            const uint32_t len = ec64_text(ks[i], text);
            h.keys.emplace_back(text, len); h.cnt.push_back(kc[i] + 1ull); h.first.push_back(kf[i]);      // (the word holds n - 1)
        }
    }
    return F2Q_OK;
}

extern "C" int f2q_ec_size(f2q_ctx *c, uint64_t *n_keys, uint64_t *n_bytes)
{
    if (!c || !n_keys || !n_bytes) return F2Q_EINVAL;
    *n_keys = 0; *n_bytes = 0;
    if (c->prm.mode != 1) return fail(c, F2Q_ESTATE, "not in Extract+Count mode");
    HIPC(c, hipSetDevice(c->device));
    EcHost h; int rc = ec_pull(c, h);
    if (rc) return rc;
    uint64_t nb = 0; for (auto &k : h.keys) nb += k.size();
    *n_keys = h.keys.size(); *n_bytes = nb;
    return F2Q_OK;
}

extern "C" int f2q_ec_fetch(f2q_ctx *c, char *keys, uint64_t *offs, int64_t *counts, uint64_t *first_read)
{
    if (!c || !offs) return F2Q_EINVAL;
    if (c->prm.mode != 1) return fail(c, F2Q_ESTATE, "not in Extract+Count mode");
    offs[0] = 0;
    HIPC(c, hipSetDevice(c->device));
    EcHost h; int rc = ec_pull(c, h);
    if (rc) return rc;
    uint64_t o = 0;
    for (size_t e = 0; e < h.keys.size(); e++) {
        if (keys) memcpy(keys + o, h.keys[e].data(), h.keys[e].size());
        o += h.keys[e].size(); offs[e + 1] = o;
        if (counts) counts[e] = (int64_t)h.cnt[e];
        if (first_read) first_read[e] = h.first[e];
    }
    return F2Q_OK;
}

// ---- Extract+Count with a library --------------------------------------------------------------------
extern "C" int f2q_set_assign_library(f2q_ctx *c, const char *seqs, const uint32_t *offs, uint32_t n)
{
    if (!c || !offs || (!seqs && n)) return fail(c, F2Q_EINVAL, "null argument");
    if (c->prm.mode != 1) return fail(c, F2Q_ESTATE, "an assign library belongs to an Extract+Count context (Counter mode: f2q_set_features)");
    if (c->have_asg) return fail(c, F2Q_ESTATE, "f2q_set_assign_library may be called once per context");
    HIPC(c, hipSetDevice(c->device));
    for (uint32_t i = 0; i < n; i++) if (offs[i + 1] < offs[i]) return fail(c, F2Q_EINVAL, "offsets must be non-decreasing");
    // the index match_key reads: the 2-bit tables by length and the byte-string index; no packed tables (no kernel of
    // this context counts against it), so the pack plan and the path choice stay what they were
    build_index(c->asg_ix, seqs ? seqs : "", offs, n, c->run_h.miss);
    int rc = upload_index(c, c->asg_ix, c->asg_lib_h, &c->asg_lib_d, c->asg_lib_allocs, nullptr);
    if (rc) return rc;
    HIPC(c, hipMalloc((void **)&c->asg_acc_d, ((size_t)n + 6) * sizeof(unsigned long long)));
    c->have_asg = true;
    return F2Q_OK;
}

extern "C" int f2q_ec_assign(f2q_ctx *c, int64_t *counts, int64_t stats[5], f2q_timing *t)
{
    if (!c) return F2Q_EINVAL;
    if (t) memset(t, 0, sizeof *t);
    if (c->prm.mode != 1) return fail(c, F2Q_ESTATE, "not in Extract+Count mode");
    if (!c->have_asg) return fail(c, F2Q_ESTATE, "f2q_set_assign_library must be called before f2q_ec_assign");
    HIPC(c, hipSetDevice(c->device));
    const uint64_t nf = c->asg_lib_h.n_features;
    // everything that still counts into the tables comes first: the raw records' stream is joined as f2q_reset_counts and
    // the table growth join it; the hot-key launches (whose workgroups add their LDS counters to the table as they end)
    // and the deferred passes are on the context's stream, ahead of the kernels below
    if (c->aux_busy) { HIPC(c, hipStreamSynchronize(c->aux_stream)); c->aux_busy = false; }
    unsigned long long ctr[F2Q_CTR_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    int rc;
    if (c->ec.ctr && (rc = ec_counters(c, ctr))) return rc;
    const uint64_t nb = c->ec.slots ? ctr[0] : 0, nw = c->ec.k64_slots ? (uint64_t)c->ec.k64_mask + 1 : 0;
    c->asg_gen = 0;
    free_all(c, c->asg_allocs);
    memset(&c->asg, 0, sizeof c->asg);
    if ((rc = dev_alloc(c, (size_t)nb, &c->asg.feat_b, c->asg_allocs))) return rc;
    if ((rc = dev_alloc(c, (size_t)nb, &c->asg.dist_b, c->asg_allocs))) return rc;
    if ((rc = dev_alloc(c, (size_t)nw, &c->asg.feat_w, c->asg_allocs))) return rc;
    if ((rc = dev_alloc(c, (size_t)nw, &c->asg.dist_w, c->asg_allocs))) return rc;
    c->asg.counts = c->asg_acc_d; c->asg.bad = c->asg_acc_d + nf + 5;
    unsigned long long *st_d = c->asg_acc_d + nf;
    // a result vector of its own, cleared by every call: assigning never adds to an earlier result
    HIPC(c, hipMemsetAsync(c->asg_acc_d, 0, (nf + 6) * sizeof(unsigned long long), c->stream));
    uint32_t launches = 0;
    HIPC(c, hipEventRecord(c->ev_k0, c->stream));
    if (nb) {
        const uint32_t grid = (uint32_t)std::min<uint64_t>((nb + F2Q_ASG_THREADS - 1) / F2Q_ASG_THREADS, (uint64_t)c->n_cu * 8u);
        hipLaunchKernelGGL(k_assign_entries, dim3(grid), dim3(F2Q_ASG_THREADS), 0, c->stream, c->run_d, c->asg_lib_d, c->ec, c->asg,
                           (unsigned long long)nb, ctr[1], st_d);
        HIPC(c, hipGetLastError());
        launches++;
        EC_POINT(c, "k_assign_entries");
    }
    if (nw && ctr[3]) {
        const uint32_t grid = (uint32_t)std::min<uint64_t>((nw + F2Q_ASG_THREADS - 1) / F2Q_ASG_THREADS, (uint64_t)c->n_cu * 8u);
        hipLaunchKernelGGL(k_assign_slots, dim3(grid), dim3(F2Q_ASG_THREADS), 0, c->stream, c->run_d, c->asg_lib_d, c->ec, c->asg, st_d);
        HIPC(c, hipGetLastError());
        launches++;
        EC_POINT(c, "k_assign_slots");
    }
    HIPC(c, hipEventRecord(c->ev_k1, c->stream));
    // reads and quality_failed are the context's own (fast2q.py:389-393 do not depend on the library)
    if (int rc = acc_ready(c)) return rc;
    HIPC(c, hipMemcpyAsync(st_d + F2Q_READS, c->acc_d + (c->acc_n - 5) + F2Q_READS, 8, hipMemcpyDeviceToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(st_d + F2Q_QUALITY_FAILED, c->acc_d + (c->acc_n - 5) + F2Q_QUALITY_FAILED, 8, hipMemcpyDeviceToDevice, c->stream));
    std::vector<unsigned long long> h(nf + 6);
    HIPC(c, hipMemcpyAsync(h.data(), c->asg_acc_d, (nf + 6) * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    if (h[nf + 5]) return fail(c, F2Q_ESTATE, std::to_string(h[nf + 5]) + " Extract+Count entries are not filled in");
    if (counts) for (uint64_t i = 0; i < nf; i++) counts[i] = (int64_t)h[i];
    if (stats) for (int k = 0; k < 5; k++) stats[k] = (int64_t)h[nf + k];
    if (t) {
        float ms = 0;
        HIPC(c, hipEventElapsedTime(&ms, c->ev_k0, c->ev_k1));
        t->kernel_ms = ms; t->total_ms = ms; t->reads = h[nf + F2Q_READS]; t->launches = launches;
    }
    // the per-key arrays cover the single-word table only when it was walked
    c->asg_nb = nb; c->asg_nw = ctr[3] ? nw : 0; c->asg_gen = c->ec_gen;
    return F2Q_OK;
}

extern "C" int f2q_ec_fetch_assigned(f2q_ctx *c, int32_t *feature, int32_t *dist)
{
    if (!c) return F2Q_EINVAL;
    if (c->prm.mode != 1) return fail(c, F2Q_ESTATE, "not in Extract+Count mode");
    if (!c->have_asg || c->asg_gen != c->ec_gen)
        return fail(c, F2Q_ESTATE, "the Extract+Count tables have changed since the last f2q_ec_assign (or it was never called)");
    HIPC(c, hipSetDevice(c->device));
    std::vector<uint32_t> fb(c->asg_nb), fw(c->asg_nw);
    std::vector<uint8_t> db(c->asg_nb), dw(c->asg_nw);
    if (c->asg_nb) {
        HIPC(c, hipMemcpyAsync(fb.data(), c->asg.feat_b, c->asg_nb * 4, hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipMemcpyAsync(db.data(), c->asg.dist_b, c->asg_nb, hipMemcpyDeviceToHost, c->stream));
    }
    if (c->asg_nw) {
        HIPC(c, hipMemcpyAsync(fw.data(), c->asg.feat_w, c->asg_nw * 4, hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipMemcpyAsync(dw.data(), c->asg.dist_w, c->asg_nw, hipMemcpyDeviceToHost, c->stream));
    }
    HIPC(c, hipStreamSynchronize(c->stream));
    // f2q_ec_fetch's order: the byte-string entries, then the occupied single-word slots
    size_t o = 0;
    auto put = [&](uint32_t f, uint8_t d) {
        if (feature) feature[o] = f == F2Q_ASG_NONE ? -1 : (int32_t)f;
        if (dist) dist[o] = d == F2Q_ASG_NODIST ? -1 : (int32_t)d;
        o++;
    };
    for (size_t e = 0; e < fb.size(); e++) put(fb[e], db[e]);
    for (size_t s = 0; s < fw.size(); s++) if (dw[s] != F2Q_ASG_EMPTY) put(fw[s], dw[s]);
    return F2Q_OK;
}

// ---- Extract+Count: extracted keys one base apart collapsed ----------------------------------------------
// A pass over the single-word table after counting (include/f2q.h: ec_collapse).  parent[], root[] and cluster[] (with the
// four counters behind it) are scratch of 16 bytes per slot from the device-memory cache; root[] and cluster[] stay until
// the next call for f2q_ec_fetch_collapsed.  The tables are only read, so the call changes nothing another call reads.
// The parent launch is the lane-per-slot k_ec_parent_lane (F2Q_ECC_LINK=lane, and the default: on the 50 M-read workload it
// measured 3 % faster than the wave-cooperative layout, profiles/r19_ec_collapse_rates.txt); F2Q_ECC_LINK=wave: k_ec_parent
// (A/B runs, cross-checks)
extern "C" int f2q_ec_collapse(f2q_ctx *c, int32_t dist, int32_t ratio, int64_t extra[4], f2q_timing *t)
{
    if (!c) return F2Q_EINVAL;
    if (t) memset(t, 0, sizeof *t);
    if (extra) memset(extra, 0, 4 * sizeof(int64_t));
    if (c->prm.mode != 1) return fail(c, F2Q_ESTATE, "not in Extract+Count mode");
    if (dist != 0 && dist != 1) return fail(c, F2Q_EINVAL, "extracted keys are collapsed at one mismatch (or 0: as they are)");
    if (ratio < 2 || ratio > 255) return fail(c, F2Q_EINVAL, "the read ratio of a parent must be 2 .. 255");
    HIPC(c, hipSetDevice(c->device));
    const double t0 = now_ms();
    // everything that still counts into the tables comes first, as in f2q_ec_assign
    if (c->aux_busy) { HIPC(c, hipStreamSynchronize(c->aux_stream)); c->aux_busy = false; }
    unsigned long long ctr[F2Q_CTR_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    int rc;
    if (c->ec.ctr && (rc = ec_counters(c, ctr))) return rc;
    const uint64_t nb = c->ec.slots ? ctr[0] : 0, nw = c->ec.k64_slots && ctr[3] && dist ? (uint64_t)c->ec.k64_mask + 1 : 0;
    c->ecc_gen = 0;
    free_all(c, c->ecc_allocs);
    c->ecc_root = nullptr; c->ecc_cluster = nullptr;
    if (nw > (1ull << 31)) return fail(c, F2Q_ENOMEM, "the single-word table has more than 2^31 slots: too large to collapse");
    unsigned long long h[F2Q_ECC_CTR_WORDS] = {0, 0, 0, 0};
    float ms = 0, ms_parent = 0;
    struct Event { hipEvent_t e = nullptr; ~Event() { if (e) (void)hipEventDestroy(e); } } mid;      // F2Q_TRACE=1: between the two kernels
    const char *e = getenv("F2Q_ECC_LINK");
    const bool by_lane = !(e && !strcmp(e, "wave"));
    uint32_t launches = 0;
    if (nw) {
        uint32_t *parent = nullptr;
        if (dev_alloc(c, (size_t)nw, &parent, c->ecc_allocs) || dev_alloc(c, (size_t)nw, &c->ecc_root, c->ecc_allocs) ||
            dev_alloc(c, (size_t)nw + F2Q_ECC_CTR_WORDS, &c->ecc_cluster, c->ecc_allocs)) {
            free_all(c, c->ecc_allocs);
            c->ecc_root = nullptr; c->ecc_cluster = nullptr;
            return fail(c, F2Q_ENOMEM, "no device memory to collapse a table of " + std::to_string(nw) + " slots: " + c->err);
        }
        HIPC(c, hipMemsetAsync(c->ecc_cluster, 0, (nw + F2Q_ECC_CTR_WORDS) * sizeof(unsigned long long), c->stream));
        const uint32_t grid = (uint32_t)std::min<uint64_t>((nw + F2Q_ECC_THREADS - 1) / F2Q_ECC_THREADS, (uint64_t)c->n_cu * 8u);
        HIPC(c, hipEventRecord(c->ev_k0, c->stream));
        if (by_lane) hipLaunchKernelGGL(k_ec_parent_lane, dim3(grid), dim3(F2Q_ECC_THREADS), 0, c->stream, c->ec, parent, (uint32_t)ratio);
        else hipLaunchKernelGGL(k_ec_parent, dim3(grid), dim3(F2Q_ECC_THREADS), 0, c->stream, c->ec, parent, (uint32_t)ratio);
        HIPC(c, hipGetLastError());
        EC_POINT(c, "k_ec_parent");
        if (c->trace) { HIPC(c, hipEventCreate(&mid.e)); HIPC(c, hipEventRecord(mid.e, c->stream)); }
        hipLaunchKernelGGL(k_ec_roots, dim3(grid), dim3(F2Q_ECC_THREADS), 0, c->stream, c->ec, (const uint32_t *)parent, c->ecc_root, c->ecc_cluster);
        HIPC(c, hipGetLastError());
        EC_POINT(c, "k_ec_roots");
        HIPC(c, hipEventRecord(c->ev_k1, c->stream));
        launches = 2;
        HIPC(c, hipMemcpyAsync(h, c->ecc_cluster + nw, sizeof h, hipMemcpyDeviceToHost, c->stream));
    }
    HIPC(c, hipStreamSynchronize(c->stream));
    if (nw) HIPC(c, hipEventElapsedTime(&ms, c->ev_k0, c->ev_k1));
    if (mid.e) HIPC(c, hipEventElapsedTime(&ms_parent, c->ev_k0, mid.e));
    if (extra) for (int k = 0; k < F2Q_ECC_CTR_WORDS; k++) extra[k] = (int64_t)h[k];
    if (t) { t->kernel_ms = ms; t->total_ms = now_ms() - t0; t->launches = launches; }
    c->ecc_nb = nb; c->ecc_nw = nw; c->ecc_gen = c->ec_gen;
    if (c->trace) fprintf(stderr, "[f2q trace] Extract+Count collapse (mismatches %d, ratio %d): %llu keys, %llu eligible, %llu absorbed with %llu reads, longest chain %llu, "
                          "%.3f ms (kernels %.3f: k_ec_parent %.3f, k_ec_roots %.3f; %s, %llu slots)\n", dist, ratio, (unsigned long long)(ctr[0] + ctr[3]), h[0], h[1], h[2], h[3],
                          now_ms() - t0, ms, ms_parent, ms - ms_parent,
                          by_lane ? "lane" : "wave", (unsigned long long)nw);
    return F2Q_OK;
}

extern "C" int f2q_ec_fetch_collapsed(f2q_ctx *c, uint64_t *centroid, int64_t *cluster_reads)
{
    if (!c) return F2Q_EINVAL;
    if (c->prm.mode != 1) return fail(c, F2Q_ESTATE, "not in Extract+Count mode");
    if (c->ecc_gen != c->ec_gen)
        return fail(c, F2Q_ESTATE, "the Extract+Count tables have changed since the last f2q_ec_collapse (or it was never called)");
    HIPC(c, hipSetDevice(c->device));
    // f2q_ec_fetch's order: the byte-string entries (each its own centroid), then the occupied single-word slots
    const size_t nb = (size_t)c->ecc_nb, ns = c->ec.k64_slots ? (size_t)c->ec.k64_mask + 1 : 0;
    std::vector<unsigned long long> cnt(nb);
    if (nb) HIPC(c, hipMemcpyAsync(cnt.data(), c->ec.ent_count, nb * 8, hipMemcpyDeviceToHost, c->stream));
    std::vector<unsigned long long> ks(ns), kc(ns), cl(c->ecc_nw);
    std::vector<uint32_t> root(c->ecc_nw);
    if (ns) {
        HIPC(c, hipMemcpyAsync(ks.data(), c->ec.k64_slots, ns * 8, hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipMemcpyAsync(kc.data(), c->ec.k64_count, ns * 8, hipMemcpyDeviceToHost, c->stream));
    }
    if (c->ecc_nw) {
        if (c->ecc_nw != ns) return fail(c, F2Q_ESTATE, "the single-word table is not the one f2q_ec_collapse walked");
        HIPC(c, hipMemcpyAsync(root.data(), c->ecc_root, ns * 4, hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipMemcpyAsync(cl.data(), c->ecc_cluster, ns * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIPC(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < nb; i++) {
        if (centroid) centroid[i] = i;
        if (cluster_reads) cluster_reads[i] = (int64_t)cnt[i];
    }
    std::vector<uint64_t> index(ns);                             // slot -> position among the occupied slots
    size_t o = nb;
    for (size_t s = 0; s < ns; s++) if (ks[s] != KEY_EMPTY) index[s] = o++;
    for (size_t s = 0; s < ns; s++) {
        if (ks[s] == KEY_EMPTY) continue;
        const bool walked = c->ecc_nw != 0;
        const size_t r = walked ? root[s] : s;
        if (r >= ns || ks[r] == KEY_EMPTY) return fail(c, F2Q_ESTATE, "slot " + std::to_string(s) + " of the single-word table has no centroid");
        if (centroid) centroid[index[s]] = index[r];
        if (cluster_reads) cluster_reads[index[s]] = (int64_t)(walked ? cl[s] : kc[s] + 1ull);      // (the count word holds n - 1)
    }
    return F2Q_OK;
}
