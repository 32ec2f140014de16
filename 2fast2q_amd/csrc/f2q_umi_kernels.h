// f2q_umi_kernels.h -- distinct UMIs per feature (--umi, f2q_set_umi; included by f2q_lib.hip only).
//   k_count_umi<READS>   Counter mode on raw records, the byte-exact routine, plus the (feature, UMI) set: one pass
//                  (<false>: the set alone; <true>: reads per pair too, f2q_set_umi_reads)
//   k_count_umi_pair<READS, STAGE>   the same on the merged records of a paired context (f2q_set_umi_paired): the UMI in
//                  one mate or split over both (UmiPairHook); STAGE: its own, wider staging area, or none
//   k_header_umi   the UMI in every record's header line (f2q_set_umi_header), at ingest: one entry per record of the block;
//                  k_count_umi<READS, true> / k_count_umi_pair<READS, STAGE, true> then take the UMI from that array
//   k_umi_rehash<READS>  the pairs of a full set into a larger one (<true>: with their reads)
//   k_umi_uf_init / k_umi_link<false> / k_umi_link_lane / k_umi_roots   UMIs at Hamming distance 1 collapsed per feature
//                  (f2q_umi_collapse): three launches over the set, the kernel boundary is the only hand-off
//   k_umi_link<true> / k_umi_dir_spread / k_umi_dir_roots   the directional rule (f2q_umi_collapse_directional), after
//                  k_umi_uf_init: four launches
// The per-lane logic (UmiDev, umi_claim_at, umi_insert, umi_rehash_one, umi_codes, UmiHook, umi_codes_paired, UmiPairHook, header_umi_codes, UmiHeaderHook, umi_find, uf_find / uf_union,
// umi_neighbour, umi_link_one, umi_root_one, umi_link_dir_one, umi_dir_spread_one, umi_dir_root_one) lives in f2q_device.h.
#pragma once

// k_count_general's shape (64-thread workgroups, the record's two lines staged in LDS, a record longer than the staging
// area walked in global memory); a read the routine assigns to a feature also brings its UMI to the set.  Single-end
// Counter mode only (f2q_set_umi refuses everything else).  The host has sized the set so that every record of the
// launch could bring a new pair and it would still be at most half full.
// READS: every read with a valid UMI also adds 1 to reads[slot of its pair] (UmiHook<P, true>); false is the only
// instance launched unless f2q_set_umi_reads asked for reads.
// HDR (f2q_set_umi_header): the UMI was read from the record's header at ingest (k_header_umi), the hook takes codes and
// validity from rb.hdr_umi[position of the record in the block] and decodes nothing; everything after the hook is the same.
template <bool READS, bool HDR = false>
__global__ __launch_bounds__(F2Q_GEN_THREADS) void k_count_umi(const RunDev *__restrict__ runp, const LibDev *__restrict__ libp,
                                                                EcDev ec, RawBlock rb, Accum acc, UmiDev umi)
{
    __shared__ uint32_t stage[F2Q_GEN_THREADS * F2Q_GEN_STRIDE];
    const RunDev &run = *runp;
    const LibDev &lib = *libp;
    unsigned long long st[5] = {0, 0, 0, 0, 0};
    unsigned long long ust[3] = {0, 0, 0};
    const auto raw = gp(rb.raw);
    uint32_t *mine = stage + threadIdx.x * F2Q_GEN_STRIDE;
    for (uint64_t i = (uint64_t)blockIdx.x * F2Q_GEN_THREADS + threadIdx.x; i < rb.n; i += (uint64_t)gridDim.x * F2Q_GEN_THREADS) {
        const unsigned long long so = gp(rb.off)[i];
        const int r = (int)gp(rb.len)[i], qn = (int)gp(rb.qlen)[i];
        const unsigned long long qo = rb.qoff ? gp(rb.qoff)[i] : so + (unsigned long long)r;
        const unsigned long long gi = rb.first_index + (rb.index ? gp(rb.index)[i] : i);
        const unsigned long long he = HDR ? gp(rb.hdr_umi)[rb.index ? gp(rb.index)[i] : i] : 0ull;
        const uint32_t ms = (uint32_t)so & 3u, mq = (uint32_t)qo & 3u;
        if (r >= 0 && qn >= 0 && ms + (uint32_t)r <= 4u * F2Q_GEN_WORDS && mq + (uint32_t)qn <= 4u * F2Q_GEN_WORDS) {
            stage_line(mine, raw, so, r);
            stage_line(mine + F2Q_GEN_WORDS, raw, qo, qn);
            const uint8_t *sl = reinterpret_cast<const uint8_t *>(mine) + ms;
            const uint8_t *ql = reinterpret_cast<const uint8_t *>(mine + F2Q_GEN_WORDS) + mq;
            if constexpr (HDR) {
                const UmiHeaderHook<READS> hook{&umi, he, ust};
                general_read<const uint8_t *, true, false>(run, lib, ec, acc, sl, r, ql, qn, gi, st, nullptr, 0, 0, hook);
            } else {
                const UmiHook<const uint8_t *, READS> hook{&umi, run.thr, sl, r, ql, qn, ust};
                general_read<const uint8_t *, true, false>(run, lib, ec, acc, sl, r, ql, qn, gi, st, nullptr, 0, 0, hook);
            }
        } else if constexpr (HDR) {
            const UmiHeaderHook<READS> hook{&umi, he, ust};
            general_read<gbytes, true, false>(run, lib, ec, acc, raw + so, r, raw + qo, qn, gi, st, nullptr, 0, 0, hook);
        } else {
            const UmiHook<gbytes, READS> hook{&umi, run.thr, raw + so, r, raw + qo, qn, ust};
            general_read<gbytes, true, false>(run, lib, ec, acc, raw + so, r, raw + qo, qn, gi, st, nullptr, 0, 0, hook);
        }
    }
    // one wave per workgroup: at most one atomic per counter
    const unsigned long long ok = wave_sum(ust[0]), bad = wave_sum(ust[1]), fresh = wave_sum(ust[2]);
    if (threadIdx.x == 0) {
        if (ok) acc_add(&umi.ctr[F2Q_UMI_READS], ok);
        if (bad) acc_add(&umi.ctr[F2Q_UMI_FAILED], bad);
        if (fresh) acc_add(&umi.ctr[F2Q_UMI_HELD], fresh);
    }
    __shared__ unsigned long long st_lds[8];
    flush_stats(acc, st, st_lds, nullptr);
}

// The paired instance (f2q_set_umi_paired): the records are merged pairs (RawBlock::len1 / qlen1 set), every pair of the
// sample comes here (the context clears its plan's fast-path flags), and the routine is general_read<.., PAIRED> with a
// UmiPairHook.  A paired context has fixed windows only, so a pair touches its windows and its UMI parts: a few dozen
// bytes of a merged record of about 600.  k_count_umi's own staging area (192 bytes per line) would send every 2 x 150
// pair down the global-memory walk, so the layout is this kernel's own, and an A/B switch (F2Q_UMI_PAIR_STAGE):
//   STAGE  the two merged lines staged in an area of F2Q_UMI_PAIR_WORDS words each (304 bytes: 2 x 150 bases at any
//          misalignment), odd word stride per lane; a longer line is walked in global memory
//   !STAGE no staging area at all: the touched bytes are read from global memory
// (which one is the default, and the measured rates: DESIGN.md).  k_count_umi itself is not touched by any of this.
#define F2Q_UMI_PAIR_WORDS 76u
#define F2Q_UMI_PAIR_STAGE_DEFAULT false
#define F2Q_UMI_PAIR_STRIDE (2u * F2Q_UMI_PAIR_WORDS + 1u)
// HDR (f2q_set_umi_header on a paired context): the UMI of a pair is the one in mate 1's header, taken from rb.hdr_umi as
// in k_count_umi<.., true>; the merged record is then read for the feature parts alone.
template <bool READS, bool STAGE, bool HDR = false>
__global__ __launch_bounds__(F2Q_GEN_THREADS) void k_count_umi_pair(const RunDev *__restrict__ runp, const LibDev *__restrict__ libp,
                                                                     EcDev ec, RawBlock rb, Accum acc, UmiDev umi)
{
    __shared__ uint32_t stage[STAGE ? F2Q_GEN_THREADS * F2Q_UMI_PAIR_STRIDE : 1u];
    const RunDev &run = *runp;
    const LibDev &lib = *libp;
    unsigned long long st[5] = {0, 0, 0, 0, 0};
    unsigned long long ust[3] = {0, 0, 0};
    const auto raw = gp(rb.raw);
    uint32_t *mine = stage + (STAGE ? threadIdx.x * F2Q_UMI_PAIR_STRIDE : 0u);
    for (uint64_t i = (uint64_t)blockIdx.x * F2Q_GEN_THREADS + threadIdx.x; i < rb.n; i += (uint64_t)gridDim.x * F2Q_GEN_THREADS) {
        const unsigned long long so = gp(rb.off)[i];
        const int r = (int)gp(rb.len)[i], qn = (int)gp(rb.qlen)[i];
        const unsigned long long qo = rb.qoff ? gp(rb.qoff)[i] : so + (unsigned long long)r;
        const unsigned long long gi = rb.first_index + (rb.index ? gp(rb.index)[i] : i);
        const int r1 = (int)gp(rb.len1)[i], qn1 = (int)gp(rb.qlen1)[i];
        const unsigned long long he = HDR ? gp(rb.hdr_umi)[rb.index ? gp(rb.index)[i] : i] : 0ull;
        const uint32_t ms = (uint32_t)so & 3u, mq = (uint32_t)qo & 3u;
        if (STAGE && r >= 0 && qn >= 0 && ms + (uint32_t)r <= 4u * F2Q_UMI_PAIR_WORDS && mq + (uint32_t)qn <= 4u * F2Q_UMI_PAIR_WORDS) {
            stage_line(mine, raw, so, r);
            stage_line(mine + F2Q_UMI_PAIR_WORDS, raw, qo, qn);
            const uint8_t *sl = reinterpret_cast<const uint8_t *>(mine) + ms;
            const uint8_t *ql = reinterpret_cast<const uint8_t *>(mine + F2Q_UMI_PAIR_WORDS) + mq;
            if constexpr (HDR) {
                const UmiHeaderHook<READS> hook{&umi, he, ust};
                general_read<const uint8_t *, true, true>(run, lib, ec, acc, sl, r, ql, qn, gi, st, nullptr, r1, qn1, hook);
            } else {
                const UmiPairHook<const uint8_t *, READS> hook{&umi, run.thr, sl, r, r1, ql, qn, qn1, ust};
                general_read<const uint8_t *, true, true>(run, lib, ec, acc, sl, r, ql, qn, gi, st, nullptr, r1, qn1, hook);
            }
        } else if constexpr (HDR) {
            const UmiHeaderHook<READS> hook{&umi, he, ust};
            general_read<gbytes, true, true>(run, lib, ec, acc, raw + so, r, raw + qo, qn, gi, st, nullptr, r1, qn1, hook);
        } else {
            const UmiPairHook<gbytes, READS> hook{&umi, run.thr, raw + so, r, r1, raw + qo, qn, qn1, ust};
            general_read<gbytes, true, true>(run, lib, ec, acc, raw + so, r, raw + qo, qn, gi, st, nullptr, r1, qn1, hook);
        }
    }
    // one wave per workgroup: at most one atomic per counter
    const unsigned long long ok = wave_sum(ust[0]), bad = wave_sum(ust[1]), fresh = wave_sum(ust[2]);
    if (threadIdx.x == 0) {
        if (ok) acc_add(&umi.ctr[F2Q_UMI_READS], ok);
        if (bad) acc_add(&umi.ctr[F2Q_UMI_FAILED], bad);
        if (fresh) acc_add(&umi.ctr[F2Q_UMI_HELD], fresh);
    }
    __shared__ unsigned long long st_lds[8];
    flush_stats(acc, st, st_lds, nullptr);
}

// every pair of `old` into `nw` (umi_rehash_one); READS: with its reads
template <bool READS>
__global__ __launch_bounds__(256) void k_umi_rehash(UmiDev old, UmiDev nw)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= old.mask) umi_rehash_one<READS>(old, nw, (uint32_t)i);
}

// ---- f2q_umi_collapse: a union-find over the slots of the set --------------------------------------------------------
// every slot its own root
__global__ __launch_bounds__(256) void k_umi_uf_init(uint32_t *parent, unsigned long long n)
{
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x)
        gpw(parent)[i] = (uint32_t)i;
}

// The set is at most half full and one pair has 3L look-ups, each a dependent probe chain of its own: a lane that
// walked its own slot's 3L neighbours would run them one after the other while the lanes of the empty slots idle.
// So a wave takes 64 consecutive slots, compacts the occupied ones into its row of LDS, and then takes them 64 / 3L
// at a time: lane g * 3L + n probes neighbour n of the g-th pair of the round, all look-ups of the round in flight
// together.  Edges are summed per wave: one atomic per wave.  Any grid: waves stride over the set.
#define F2Q_UMI_LINK_THREADS 256
#define F2Q_UMI_LINK_WG_DEFAULT 256
#define F2Q_UMI_LINK_GRID_DEFAULT 8
// DIR: the directional rule (f2q_umi_collapse_directional) -- the pair's reads travel next to its word in the wave's row
// (cnts; one row in the other instance, never touched) and dom[] (null otherwise) takes the flags.  slots[] and reads[]
// are written by earlier launches only (plain loads); parent[] is accessed by agent-scope atomics inside uf_union;
// dom[] is only written here (F2Q_ST32, every writer stores the same 1) and read by the launches after this one.
template <bool DIR>
__global__ __launch_bounds__(F2Q_UMI_LINK_THREADS) void k_umi_link(UmiDev u, uint32_t *parent, uint32_t *dom, unsigned long long *edges)
{
    __shared__ unsigned long long keys[F2Q_UMI_LINK_THREADS / 64][64];
    __shared__ uint32_t cnts[DIR ? F2Q_UMI_LINK_THREADS / 64 : 1][64];
    __shared__ uint8_t from[F2Q_UMI_LINK_THREADS / 64][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const uint32_t per = 3u * (uint32_t)u.length, groups = 64u / per;
    const uint32_t g = lane / per, n = lane - g * per;
    const unsigned long long slots = (unsigned long long)u.mask + 1ull;
    unsigned long long found = 0;
    for (unsigned long long base = ((unsigned long long)blockIdx.x * waves + wave) * 64ull; base < slots; base += (unsigned long long)gridDim.x * waves * 64ull) {
        const unsigned long long k = base + lane < slots ? gp(u.slots)[base + lane] : KEY_EMPTY;
        const unsigned long long occ = __ballot(k != KEY_EMPTY);
        if (occ == 0ull) continue;
        if (k != KEY_EMPTY) {
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(occ >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)occ, 0u));
            keys[wave][rank] = k; from[wave][rank] = (uint8_t)lane;
            if (DIR) cnts[wave][rank] = gp(u.reads)[base + lane];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const uint32_t cnt = (uint32_t)__popcll(occ);
        for (uint32_t t = 0; t < cnt; t += groups) {
            const uint32_t q = t + g;
            if (g < groups && q < cnt) {
                const uint32_t i = (uint32_t)base + from[wave][q];
                if (DIR) found += umi_link_dir_one(u, parent, dom, i, keys[wave][q], cnts[wave][q], n);
                else found += umi_link_one(u, parent, i, keys[wave][q], n);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    found = wave_sum(found);
    if (lane == 0 && found) acc_add(edges, found);
}

// the plain layout, kept for the comparison (F2Q_UMI_LINK=lane): a lane per slot, its 3L look-ups one after the other
__global__ __launch_bounds__(F2Q_UMI_LINK_THREADS) void k_umi_link_lane(UmiDev u, uint32_t *parent, unsigned long long *edges)
{
    const uint32_t per = 3u * (uint32_t)u.length;
    const unsigned long long slots = (unsigned long long)u.mask + 1ull;
    unsigned long long found = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long k = gp(u.slots)[i];
        if (k == KEY_EMPTY) continue;
        for (uint32_t n = 0; n < per; n++) found += umi_link_one(u, parent, (uint32_t)i, k, n);
    }
    found = wave_sum(found);
    if ((threadIdx.x & 63u) == 0 && found) acc_add(edges, found);
}

// after k_umi_link has ended (parent[] is stable): every root adds 1 to the molecules of its feature
__global__ __launch_bounds__(256) void k_umi_roots(UmiDev u, uint32_t *parent, unsigned long long *molecules)
{
    const unsigned long long slots = (unsigned long long)u.mask + 1ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (unsigned long long)gridDim.x * blockDim.x)
        umi_root_one(u, parent, molecules, (uint32_t)i);
}

// ---- f2q_umi_collapse_directional -------------------------------------------------------------------------------------
// after k_umi_link<true> has ended: parent[] is stable, so is bit 0 of every dom[].  A dominated single-read slot that is
// not its own root ORs bit 1 into dom[root].  Only roots are written and only the flags of slots that are no roots decide
// anything here, so no lane reads what another lane of this launch writes; k_umi_dir_roots reads the result.
__global__ __launch_bounds__(256) void k_umi_dir_spread(UmiDev u, const uint32_t *parent, uint32_t *dom)
{
    const unsigned long long slots = (unsigned long long)u.mask + 1ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (unsigned long long)gridDim.x * blockDim.x)
        umi_dir_spread_one(u, parent, dom, (uint32_t)i);
}

// after k_umi_dir_spread has ended: the molecules per feature; tot[0] += slots the link flagged, tot[1] += reads held
__global__ __launch_bounds__(256) void k_umi_dir_roots(UmiDev u, const uint32_t *parent, const uint32_t *dom, unsigned long long *molecules,
                                                       unsigned long long *tot)
{
    const unsigned long long slots = (unsigned long long)u.mask + 1ull;
    unsigned long long mine[2] = {0, 0};
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (unsigned long long)gridDim.x * blockDim.x)
        umi_dir_root_one(u, parent, dom, molecules, (uint32_t)i, mine);
    const unsigned long long flagged = wave_sum(mine[0]), reads = wave_sum(mine[1]);
    if ((threadIdx.x & 63u) == 0) {
        if (flagged) acc_add(&tot[0], flagged);
        if (reads) acc_add(&tot[1], reads);
    }
}

// ---- f2q_set_umi_header: the UMI in the header line ------------------------------------------------------------------
// After frame_text_device, on the text the raw records point into (a pair: mate 1's text).  k_classify's pattern: the 64
// records of a wave are neighbours in the text, so the wave copies the stretch from its first header to the end of its last
// one into LDS once (stage_span: 16-byte loads, every byte fetched once) and each lane walks its own header there
// (header_umi_codes); a stretch longer than the staging area is walked in global memory.  out[r] = the entry of record r
// (RawBlock::hdr_umi).  Line 4r is never the text's last line (the record is complete), so line_start[4r + 1] - 1 is the
// header's '\n' itself and every byte read lies inside the text.
struct HeaderUmiDev {
    const uint8_t *text; const uint32_t *line_start; uint32_t n_records;
    uint32_t sep, length;
    unsigned long long *out;                     // [n_records]
};
__global__ __launch_bounds__(F2Q_ING_THREADS) void k_header_umi(HeaderUmiDev d)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[F2Q_ING_LDS];
    const uint32_t r0 = blockIdx.x * F2Q_ING_THREADS, r = r0 + threadIdx.x;
    const uint32_t n_act = d.n_records - r0 < F2Q_ING_THREADS ? d.n_records - r0 : F2Q_ING_THREADS;
    const bool live = r < d.n_records;
    const auto ls = gp(d.line_start);
    const uint32_t rr = live ? r : d.n_records - 1u;
    const uint32_t s = ls[4u * rr], e = ls[4u * rr + 1u] - 1u;
    const uint32_t lo = __shfl(s, 0, 64), hi = __shfl(e, (int)n_act - 1, 64);
    const bool fits = hi >= lo && hi - (lo & ~15u) <= F2Q_ING_LDS;
    unsigned long long entry = 0;
    if (fits) {
        stage_span(stage, gp(d.text), lo, hi);
        if (live) entry = header_umi_entry<const uint8_t *>(stage + (s - (lo & ~15u)), e - s, d.sep, d.length);
    } else if (live) entry = header_umi_entry<gbytes>(gp(d.text) + s, e - s, d.sep, d.length);
    if (live) gpw(d.out)[r] = entry;
}
