// f2q_pair_kernels.h -- device-side ingest of paired-end FASTQ (included by f2q_lib.hip only, after f2q_aux_kernels.h).
// Record i of text 1 pairs with record i of text 2 (headers are not compared, as fast2q.py:324-328 never looks at them).
// Both texts are framed by k_nl_count / k_line_starts; k_classify_paired applies fastq_parser's framing to both mates and
// decides per pair whether a compact tile can carry it; k_pack_paired lays clean pairs into tiles -- mate-1 windows first,
// mate-2 windows behind them, mate 2 read from its end and complemented under rc2, so the slot is the one the merged
// read would get and every counting kernel runs as it is -- and writes every other pair as a merged raw record
// (mate 1 + mate 2 as the run takes it, sequence then quality) for the byte-exact routine (general_read<.., PAIRED>).
#pragma once

// One wave = 64 neighbouring pairs; the wave's stretch of EACH text goes into its half of the 40 KiB staging area with
// 16-byte loads (stage_span), so each byte of either text is fetched once.  A half holds 64 records of up to 320 bytes
// (150-base mates with short headers); when the 64 do not fit, the wave works in two passes of 32 pairs (records of up to
// 640 bytes: 250-base mates with Illumina headers), and a pass whose stretch still does not fit walks global memory.
#define F2Q_PAIR_LDS (F2Q_ING_LDS / 2u)

// the pairs of a wave in passes: [g0, g0 + G) with G = 64 when both stretches of the whole wave fit their areas, else 32
struct PairSpan { uint32_t lo1, hi1, lo2, hi2; bool fits; };
__device__ __forceinline__ PairSpan pair_span(uint32_t lo1_lane, uint32_t hi1_lane, uint32_t lo2_lane, uint32_t hi2_lane, uint32_t first, uint32_t last)
{
    PairSpan sp;
    sp.lo1 = __shfl(lo1_lane, (int)first, 64); sp.hi1 = __shfl(hi1_lane, (int)last, 64);
    sp.lo2 = __shfl(lo2_lane, (int)first, 64); sp.hi2 = __shfl(hi2_lane, (int)last, 64);
    sp.fits = sp.hi1 >= sp.lo1 && sp.hi1 - (sp.lo1 & ~15u) <= F2Q_PAIR_LDS && sp.hi2 >= sp.lo2 && sp.hi2 - (sp.lo2 & ~15u) <= F2Q_PAIR_LDS;
    return sp;
}

struct PairIngestDev {
    const uint8_t *text1, *text2; const uint32_t *ls1, *ls2; uint32_t n_pairs;
    // per pair and mate: sequence / quality line (offset in its text, rstrip()-ed length)
    uint32_t *off1, *len1, *qoff1, *qlen1, *off2, *len2, *qoff2, *qlen2;
    uint32_t *clean;                             // per pair: 1 = goes into the tiles
    uint32_t *raw_bytes;                         // per pair: bytes of its merged raw record (0 for a clean pair)
    uint32_t *meta;                              // [0] longest packed length among clean pairs
};

__global__ __launch_bounds__(F2Q_ING_THREADS) void k_classify_paired(PairIngestDev d, PackPlan pl)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage1[F2Q_PAIR_LDS];
    __shared__ __attribute__((aligned(16))) uint8_t stage2[F2Q_PAIR_LDS];
    const uint32_t r0 = blockIdx.x * F2Q_ING_THREADS, r = r0 + threadIdx.x;
    const uint32_t n_act = d.n_pairs - r0 < F2Q_ING_THREADS ? d.n_pairs - r0 : F2Q_ING_THREADS;
    const bool live = r < d.n_pairs;
    const uint32_t rr = live ? r : d.n_pairs - 1u;
    const auto la = gp(d.ls1), lb = gp(d.ls2);
    const uint32_t s0a = la[4u * rr + 1u], e0a = la[4u * rr + 2u] - 1u, s1a = la[4u * rr + 3u], e1a = la[4u * rr + 4u] - 1u;
    const uint32_t s0b = lb[4u * rr + 1u], e0b = lb[4u * rr + 2u] - 1u, s1b = lb[4u * rr + 3u], e1b = lb[4u * rr + 4u] - 1u;
    bool clean = false; uint32_t len1 = 0, qlen1 = 0, len2 = 0, qlen2 = 0, plen = 0;
    const uint32_t G = pair_span(s0a, e1a, s0b, e1b, 0u, n_act - 1u).fits ? 64u : 32u;
    for (uint32_t g0 = 0; g0 < n_act; g0 += G) {
        const uint32_t last = (g0 + G < n_act ? g0 + G : n_act) - 1u;
        const PairSpan sp = pair_span(s0a, e1a, s0b, e1b, g0, last);
        const bool mine = live && threadIdx.x >= g0 && threadIdx.x <= last;
        if (sp.fits) {
            stage_span(stage1, gp(d.text1), sp.lo1, sp.hi1);
            stage_span(stage2, gp(d.text2), sp.lo2, sp.hi2);
            if (mine) {
                const uint8_t *sa = stage1 + (s0a - (sp.lo1 & ~15u)), *qa = stage1 + (s1a - (sp.lo1 & ~15u));
                const uint8_t *sb = stage2 + (s0b - (sp.lo2 & ~15u)), *qb = stage2 + (s1b - (sp.lo2 & ~15u));
                len1 = rstrip_dev(sa, e0a - s0a); qlen1 = rstrip_dev(qa, e1a - s1a);
                len2 = rstrip_dev(sb, e0b - s0b); qlen2 = rstrip_dev(qb, e1b - s1b);
                const PairRecT<const uint8_t *> rec = pair_rec<const uint8_t *>(pl.rc2, sa, qa, len1, qlen1, sb, qb, len2, qlen2);
                clean = read_is_clean(pl, rec); plen = packed_len(pl, rec);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");       // the next pass overwrites the areas
        } else if (mine) {
            const gbytes sa = gp(d.text1) + s0a, qa = gp(d.text1) + s1a, sb = gp(d.text2) + s0b, qb = gp(d.text2) + s1b;
            len1 = rstrip_dev(sa, e0a - s0a); qlen1 = rstrip_dev(qa, e1a - s1a);
            len2 = rstrip_dev(sb, e0b - s0b); qlen2 = rstrip_dev(qb, e1b - s1b);
            const PairRecT<gbytes> rec = pair_rec<gbytes>(pl.rc2, sa, qa, len1, qlen1, sb, qb, len2, qlen2);
            clean = read_is_clean(pl, rec); plen = packed_len(pl, rec);
        }
    }
    if (live) {
        gpw(d.off1)[r] = s0a; gpw(d.len1)[r] = len1; gpw(d.qoff1)[r] = s1a; gpw(d.qlen1)[r] = qlen1;
        gpw(d.off2)[r] = s0b; gpw(d.len2)[r] = len2; gpw(d.qoff2)[r] = s1b; gpw(d.qlen2)[r] = qlen2;
        gpw(d.clean)[r] = clean ? 1u : 0u;
        gpw(d.raw_bytes)[r] = clean ? 0u : len1 + len2 + qlen1 + qlen2;
    }
    // the longest packed pair: one atomic per wave
    uint32_t m = (live && clean) ? plen : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const uint32_t o = __shfl_down(m, off, 64); m = o > m ? o : m; }
    if (threadIdx.x == 0 && m) atomicMax(&d.meta[0], m);
}

struct PairPackOut {
    uint32_t *bases, *qual; uint16_t *len; uint32_t *c_index; uint32_t wb, wq;
    uint8_t *raw;                                // merged raw records, back to back
    unsigned long long *g_off; uint32_t *g_len, *g_qlen, *g_len1, *g_qlen1, *g_index;
};

// one pair that the tiles cannot carry -> its merged raw record at dst: mate 1's sequence, mate 2's as the run takes it,
// then the two quality lines the same way
template <class P>
__device__ __forceinline__ void write_merged(uint8_t F2Q_GLOBAL *dst, const PairRecT<P> &rec)
{
    for (uint32_t k = 0; k < rec.len; k++) dst[k] = rec.seq[k];
    dst += rec.len;
    for (uint32_t k = 0; k < rec.len2; k++) dst[k] = rec.seq[k | F2Q_SRC_MATE2];
    dst += rec.len2;
    for (uint32_t k = 0; k < rec.qlen; k++) dst[k] = rec.qual[k];
    dst += rec.qlen;
    for (uint32_t k = 0; k < rec.qlen2; k++) dst[k] = rec.qual[k | F2Q_SRC_MATE2];
}

// clean_before / raw_before = exclusive prefix sums of PairIngestDev::clean / raw_bytes
__global__ __launch_bounds__(F2Q_ING_THREADS) void k_pack_paired(PairIngestDev d, PackPlan pl, const uint32_t *clean_before,
                                                                  const uint32_t *raw_before, PairPackOut o)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage1[F2Q_PAIR_LDS];
    __shared__ __attribute__((aligned(16))) uint8_t stage2[F2Q_PAIR_LDS];
    const uint32_t r0 = blockIdx.x * F2Q_ING_THREADS, r = r0 + threadIdx.x;
    const uint32_t n_act = d.n_pairs - r0 < F2Q_ING_THREADS ? d.n_pairs - r0 : F2Q_ING_THREADS;
    const bool live = r < d.n_pairs;
    const uint32_t rr = live ? r : d.n_pairs - 1u;
    const uint32_t off1 = gp(d.off1)[rr], qoff1 = gp(d.qoff1)[rr], len1 = gp(d.len1)[rr], qlen1 = gp(d.qlen1)[rr];
    const uint32_t off2 = gp(d.off2)[rr], qoff2 = gp(d.qoff2)[rr], len2 = gp(d.len2)[rr], qlen2 = gp(d.qlen2)[rr];
    const bool clean = live && gp(d.clean)[rr] != 0u;
    const uint32_t slot = gp(clean_before)[rr], raw_at = gp(raw_before)[rr];
    const uint64_t tile = slot / F2Q_TILE, lane = slot % F2Q_TILE;
    DevSink sink{gpw(o.bases) + tile * o.wb * F2Q_TILE + lane, gpw(o.qual) + tile * o.wq * F2Q_TILE + lane,
                 gpw(o.len) + tile * F2Q_TILE + lane};
    const uint32_t g = r - slot;
    uint8_t F2Q_GLOBAL *dst = gpw(o.raw) + raw_at;
    // the stretch of each text the pass's pairs lie in (clean pairs are packed from it, the others copied out of it)
    const uint32_t end1 = qoff1 + qlen1, end2 = qoff2 + qlen2;
    const uint32_t G = pair_span(off1, end1, off2, end2, 0u, n_act - 1u).fits ? 64u : 32u;
    for (uint32_t g0 = 0; g0 < n_act; g0 += G) {
        const uint32_t last = (g0 + G < n_act ? g0 + G : n_act) - 1u;
        const PairSpan sp = pair_span(off1, end1, off2, end2, g0, last);
        const bool mine = live && threadIdx.x >= g0 && threadIdx.x <= last;
        if (sp.fits) {
            stage_span(stage1, gp(d.text1), sp.lo1, sp.hi1);
            stage_span(stage2, gp(d.text2), sp.lo2, sp.hi2);
            if (mine) {
                const uint32_t a0 = sp.lo1 & ~15u, b0 = sp.lo2 & ~15u;
                const PairRecT<const uint8_t *> rec = pair_rec<const uint8_t *>(pl.rc2, stage1 + (off1 - a0), stage1 + (qoff1 - a0), len1, qlen1,
                                                                                stage2 + (off2 - b0), stage2 + (qoff2 - b0), len2, qlen2);
                if (clean) pack_read(pl, rec, 0u, sink); else write_merged(dst, rec);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");       // the next pass overwrites the areas
        } else if (mine) {
            const PairRecT<gbytes> rec = pair_rec<gbytes>(pl.rc2, gp(d.text1) + off1, gp(d.text1) + qoff1, len1, qlen1,
                                                          gp(d.text2) + off2, gp(d.text2) + qoff2, len2, qlen2);
            if (clean) pack_read(pl, rec, 0u, sink); else write_merged(dst, rec);
        }
    }
    if (!live) return;
    if (clean) { if (o.c_index) gpw(o.c_index)[slot] = r; }
    else {
        gpw(o.g_off)[g] = raw_at; gpw(o.g_len)[g] = len1 + len2; gpw(o.g_qlen)[g] = qlen1 + qlen2;
        gpw(o.g_len1)[g] = len1; gpw(o.g_qlen1)[g] = qlen1; gpw(o.g_index)[g] = r;
    }
}
