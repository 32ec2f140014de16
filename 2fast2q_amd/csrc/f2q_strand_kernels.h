// f2q_strand_kernels.h -- single reads counted on the reverse strand, or on whichever strand carries a feature (--strand,
// f2q_set_strand; included by f2q_lib.hip only).
//   k_count_strand<BOTH>   Counter mode on raw records, the byte-exact routine run on the record as written and / or on
//                  its mirror image: counts and the five reference counters by the rule of include/f2q.h, rev_counts per
//                  feature and the four strand counters (<true>: forward first, then reverse; <false>: reverse only)
// The per-lane logic (StrandDev, mirror_line, StrandBytes, strand_read, StrandHook) lives in f2q_device.h.
#pragma once

// k_count_umi's shape: 64-thread workgroups, the record's two lines staged in LDS, a record longer than the staging area
// walked in global memory (through StrandBytes, which mirrors on the fly).  A staged record is mirrored in place in its
// lane's words of LDS, so both trips run the routine on LDS pointers; strand_read holds the routine's one call site per
// layout.  A lane leaves the loop of trips as soon as its read is decided, so a wave whose lanes were all assigned on the
// forward strand never enters the second trip.  Single-end Counter mode only (f2q_set_strand refuses everything else).
template <bool BOTH>
__global__ __launch_bounds__(F2Q_GEN_THREADS) void k_count_strand(const RunDev *__restrict__ runp, const LibDev *__restrict__ libp,
                                                                   EcDev ec, RawBlock rb, Accum acc, StrandDev sd)
{
    __shared__ uint32_t stage[F2Q_GEN_THREADS * F2Q_GEN_STRIDE];
    const RunDev &run = *runp;
    const LibDev &lib = *libp;
    unsigned long long st[5] = {0, 0, 0, 0, 0};
    unsigned long long ext[4] = {0, 0, 0, 0};
    const auto raw = gp(rb.raw);
    uint32_t *mine = stage + threadIdx.x * F2Q_GEN_STRIDE;
    for (uint64_t i = (uint64_t)blockIdx.x * F2Q_GEN_THREADS + threadIdx.x; i < rb.n; i += (uint64_t)gridDim.x * F2Q_GEN_THREADS) {
        const unsigned long long so = gp(rb.off)[i];
        const int r = (int)gp(rb.len)[i], qn = (int)gp(rb.qlen)[i];
        const unsigned long long qo = rb.qoff ? gp(rb.qoff)[i] : so + (unsigned long long)r;
        const unsigned long long gi = rb.first_index + (rb.index ? gp(rb.index)[i] : i);
        const uint32_t ms = (uint32_t)so & 3u, mq = (uint32_t)qo & 3u;
        const bool staged = r >= 0 && qn >= 0 && ms + (uint32_t)r <= 4u * F2Q_GEN_WORDS && mq + (uint32_t)qn <= 4u * F2Q_GEN_WORDS;
        if (staged) {
            stage_line(mine, raw, so, r);
            stage_line(mine + F2Q_GEN_WORDS, raw, qo, qn);
        }
        strand_read<BOTH, gbytes>(run, lib, ec, acc, sd, staged ? mine : nullptr, mine + F2Q_GEN_WORDS, ms, mq, raw + so, raw + qo, r, qn, gi, st, ext);
    }
    // one wave per workgroup: at most one atomic per strand counter
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const unsigned long long v = wave_sum(ext[k]);
        if (threadIdx.x == 0 && v) acc_add(&sd.extra[k], v);
    }
    __shared__ unsigned long long st_lds[8];
    flush_stats(acc, st, st_lds, nullptr);
}
