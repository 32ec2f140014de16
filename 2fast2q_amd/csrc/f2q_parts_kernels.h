// f2q_parts_kernels.h -- pair libraries with each part matched alone, recombinants counted (--parts, f2q_set_parts;
// included by f2q_lib.hip only).
//   k_count_parts<PAIRED>   Counter mode on raw records, the byte-exact routine for the joined verdict, plus per read the
//                  two part verdicts: parts_counts per feature, the two marginals, the six class counters and the
//                  recombinant set with its reads (<false>: single reads, --st a,b; <true>: merged pairs, --st a --st2 b)
// The per-lane logic (PartsDev, part_verdict, parts_class, parts_pair_find, parts_read) lives in f2q_device.h, the table
// builder (parts_validate, parts_build) in f2q_host.h.  The set grows between launches through k_umi_rehash<true>.
#pragma once

// k_count_general<PAIRED>'s shape: 64-thread workgroups, the record's two lines staged in LDS, a record longer than the
// staging area walked in global memory; merged records carry mate 1's share in rb.len1 / rb.qlen1.  The host has sized the
// recombinant set so that every record of the launch could bring a new pair and it would still be at most half full.
template <bool PAIRED>
__global__ __launch_bounds__(F2Q_GEN_THREADS) void k_count_parts(const RunDev *__restrict__ runp, const LibDev *__restrict__ libp,
                                                                  EcDev ec, RawBlock rb, Accum acc, PartsDev pd)
{
    __shared__ uint32_t stage[F2Q_GEN_THREADS * F2Q_GEN_STRIDE];
    const RunDev &run = *runp;
    const LibDev &lib = *libp;
    unsigned long long st[5] = {0, 0, 0, 0, 0};
    unsigned long long cst[F2Q_PARTS_CLASSES + 1] = {0, 0, 0, 0, 0, 0, 0};
    const auto raw = gp(rb.raw);
    uint32_t *mine = stage + threadIdx.x * F2Q_GEN_STRIDE;
    for (uint64_t i = (uint64_t)blockIdx.x * F2Q_GEN_THREADS + threadIdx.x; i < rb.n; i += (uint64_t)gridDim.x * F2Q_GEN_THREADS) {
        const unsigned long long so = gp(rb.off)[i];
        const int r = (int)gp(rb.len)[i], qn = (int)gp(rb.qlen)[i];
        const unsigned long long qo = rb.qoff ? gp(rb.qoff)[i] : so + (unsigned long long)r;
        const unsigned long long gi = rb.first_index + (rb.index ? gp(rb.index)[i] : i);
        const int r1 = PAIRED ? (int)gp(rb.len1)[i] : 0, qn1 = PAIRED ? (int)gp(rb.qlen1)[i] : 0;
        const uint32_t ms = (uint32_t)so & 3u, mq = (uint32_t)qo & 3u;
        if (r >= 0 && qn >= 0 && ms + (uint32_t)r <= 4u * F2Q_GEN_WORDS && mq + (uint32_t)qn <= 4u * F2Q_GEN_WORDS) {
            stage_line(mine, raw, so, r);
            stage_line(mine + F2Q_GEN_WORDS, raw, qo, qn);
            const uint8_t *sl = reinterpret_cast<const uint8_t *>(mine) + ms;
            const uint8_t *ql = reinterpret_cast<const uint8_t *>(mine + F2Q_GEN_WORDS) + mq;
            parts_read<const uint8_t *, PAIRED>(run, lib, ec, acc, pd, sl, r, ql, qn, gi, st, cst, r1, qn1);
        } else {
            parts_read<gbytes, PAIRED>(run, lib, ec, acc, pd, raw + so, r, raw + qo, qn, gi, st, cst, r1, qn1);
        }
    }
    // one wave per workgroup: at most one atomic per class counter, one for the pairs the set gained
#pragma unroll
    for (int k = 0; k < F2Q_PARTS_CLASSES; k++) {
        const unsigned long long v = wave_sum(cst[k]);
        if (threadIdx.x == 0 && v) acc_add(&pd.classes[k], v);
    }
    const unsigned long long fresh = wave_sum(cst[F2Q_PARTS_CLASSES]);
    if (threadIdx.x == 0 && fresh) acc_add(&pd.rec.ctr[F2Q_UMI_HELD], fresh);
    __shared__ unsigned long long st_lds[8];
    flush_stats(acc, st, st_lds, nullptr);
}
