// f2q_indel_kernels.h -- reads whose feature carries one inserted or deleted base (--indel, f2q_set_indel; included by
// f2q_lib.hip only).
//   k_count_indel   Counter mode on raw records: counts and the five reference counters as k_count_general leaves them,
//                  plus, for every read the plain rule assigns nothing, the trial of include/f2q.h (indel_verdict): deletion
//                  and insertion reads per feature, per position, and the four totals
// The per-lane logic (IndelDev, indel_span_bytes, indel_decide, indel_read) lives in f2q_device.h, the builder of the
// deletion-variant table (indel_build) in f2q_host.h.
#pragma once

// k_count_stagger's shape: 64-thread workgroups, the record's two lines staged in LDS, a record longer than the staging
// area read where it lies in global memory.  The two [L] position histograms and the four totals are u32 counters in LDS
// (a counter holds the reads of ONE workgroup of ONE launch: it cannot wrap) and are added to the context's words when
// the kernel ends; the per-feature counts go straight to global memory (indel reads are rare).  Single-end Counter mode,
// one window, 2 <= L <= 31 (f2q_set_indel refuses the rest), so pos < L <= F2Q_REG_MAXLEN.
#define F2Q_INDEL_LDS (2u * F2Q_REG_MAXLEN + F2Q_INDEL_TOTALS)
__global__ __launch_bounds__(F2Q_GEN_THREADS) void k_count_indel(const RunDev *__restrict__ runp, const LibDev *__restrict__ libp,
                                                                  EcDev ec, RawBlock rb, Accum acc, IndelDev idv)
{
    __shared__ uint32_t stage[F2Q_GEN_THREADS * F2Q_GEN_STRIDE];
    __shared__ uint32_t tally[F2Q_INDEL_LDS];                    // del_pos[31], ins_pos[31], totals[4]
    const RunDev &run = *runp;
    const LibDev &lib = *libp;
    for (uint32_t i = threadIdx.x; i < F2Q_INDEL_LDS; i += F2Q_GEN_THREADS) tally[i] = 0u;
    __syncthreads();
    unsigned long long st[5] = {0, 0, 0, 0, 0};
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
        uint32_t id = 0; int pos = 0;
        const int v = indel_read<gbytes>(run, lib, ec, acc, idv, staged ? mine : nullptr, mine + F2Q_GEN_WORDS, ms, mq, raw + so, raw + qo, r, qn, gi, st, id, pos);
        if (v == F2Q_INDEL_NOT_TRIED) continue;
        atomicAdd(&tally[2u * F2Q_REG_MAXLEN], 1u);
        if (v == F2Q_INDEL_DEL) {
            acc_add(&idv.del_counts[id], 1ull);
            atomicAdd(&tally[(uint32_t)pos], 1u);
            atomicAdd(&tally[2u * F2Q_REG_MAXLEN + 1u], 1u);
        } else if (v == F2Q_INDEL_INS) {
            acc_add(&idv.ins_counts[id], 1ull);
            atomicAdd(&tally[F2Q_REG_MAXLEN + (uint32_t)pos], 1u);
            atomicAdd(&tally[2u * F2Q_REG_MAXLEN + 2u], 1u);
        } else if (v == F2Q_INDEL_AMBIGUOUS) atomicAdd(&tally[2u * F2Q_REG_MAXLEN + 3u], 1u);
    }
    __syncthreads();
    const uint32_t L = (uint32_t)run.length;
    for (uint32_t i = threadIdx.x; i < F2Q_INDEL_LDS; i += F2Q_GEN_THREADS) {
        const uint32_t v = tally[i];
        if (!v) continue;
        if (i < F2Q_REG_MAXLEN) { if (i < L) acc_add(&idv.del_pos[i], (unsigned long long)v); }
        else if (i < 2u * F2Q_REG_MAXLEN) { if (i - F2Q_REG_MAXLEN < L) acc_add(&idv.ins_pos[i - F2Q_REG_MAXLEN], (unsigned long long)v); }
        else acc_add(&idv.totals[i - 2u * F2Q_REG_MAXLEN], (unsigned long long)v);
    }
    __shared__ unsigned long long st_lds[8];
    flush_stats(acc, st, st_lds, nullptr);
}
