// f2q_stagger_kernels.h -- staggered libraries: one fixed window tried at the starts s .. s + n (--stagger,
// f2q_set_stagger; included by f2q_lib.hip only).
//   k_count_stagger   Counter mode on raw records: counts and the five reference counters by the rule of include/f2q.h
//                  (the earliest exact start, else the earliest start within --m, else what start s says), plus the reads
//                  assigned perfectly / imperfectly at each offset
// The per-lane logic (StaggerDev, stagger_walk, stagger_span, stagger_spanned, stagger_read) lives in f2q_device.h.
#pragma once

// k_count_strand's shape: 64-thread workgroups, the record's two lines staged in LDS, a record longer than the staging
// area walked in global memory.  A staged record takes the span layout where it applies (stagger_read decides), so its
// n + 1 exact probes come from registers; StaggerDev::walk sends every record through the walk layout instead.  The two
// [n + 1] histograms are u32 counters in LDS (a counter holds the reads of ONE workgroup of ONE launch: it cannot wrap)
// and are added to sd.hist when the kernel ends.  Single-end Counter mode, one window (f2q_set_stagger refuses the rest).
__global__ __launch_bounds__(F2Q_GEN_THREADS) void k_count_stagger(const RunDev *__restrict__ runp, const LibDev *__restrict__ libp,
                                                                    RawBlock rb, Accum acc, StaggerDev sd)
{
    __shared__ uint32_t stage[F2Q_GEN_THREADS * F2Q_GEN_STRIDE];
    __shared__ uint32_t hist[2 * (F2Q_STAGGER_MAX + 1)];
    const RunDev &run = *runp;
    const LibDev &lib = *libp;
    const uint32_t n_off = (uint32_t)sd.n + 1u;
    for (uint32_t i = threadIdx.x; i < 2u * n_off; i += F2Q_GEN_THREADS) hist[i] = 0u;
    __syncthreads();
    unsigned long long st[5] = {0, 0, 0, 0, 0};
    const auto raw = gp(rb.raw);
    uint32_t *mine = stage + threadIdx.x * F2Q_GEN_STRIDE;
    for (uint64_t i = (uint64_t)blockIdx.x * F2Q_GEN_THREADS + threadIdx.x; i < rb.n; i += (uint64_t)gridDim.x * F2Q_GEN_THREADS) {
        const unsigned long long so = gp(rb.off)[i];
        const int r = (int)gp(rb.len)[i], qn = (int)gp(rb.qlen)[i];
        const unsigned long long qo = rb.qoff ? gp(rb.qoff)[i] : so + (unsigned long long)r;
        const uint32_t ms = (uint32_t)so & 3u, mq = (uint32_t)qo & 3u;
        const bool staged = r >= 0 && qn >= 0 && ms + (uint32_t)r <= 4u * F2Q_GEN_WORDS && mq + (uint32_t)qn <= 4u * F2Q_GEN_WORDS;
        if (staged) {
            stage_line(mine, raw, so, r);
            stage_line(mine + F2Q_GEN_WORDS, raw, qo, qn);
        }
        uint32_t id = 0; int off = -1;
        const int v = stagger_read<gbytes>(run, lib, sd, staged ? mine : nullptr, mine + F2Q_GEN_WORDS, ms, mq, raw + so, raw + qo, r, qn, id, off);
        st[0]++;
        st[v]++;                                                 // 1 perfect, 2 imperfect, 3 non-aligned, 4 quality failed
        if (v <= 2) {
            acc_add(&acc.counts[id], 1ull);
            atomicAdd(&hist[(uint32_t)(v - 1) * n_off + (uint32_t)off], 1u);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 2u * n_off; i += F2Q_GEN_THREADS) {
        const uint32_t v = hist[i];
        if (v) acc_add(&sd.hist[i], (unsigned long long)v);
    }
    __shared__ unsigned long long st_lds[8];
    flush_stats(acc, st, st_lds, nullptr);
}
