// f2q_demux_kernels.h -- pooled samples demultiplexed by an inline barcode while they are counted (--sb,
// f2q_set_sample_barcodes; included by f2q_lib.hip only).
//   k_count_demux<LDS_TABLE>   Counter mode on raw records, the byte-exact routine, plus per read the barcode verdict:
//                  the count matrix [sample][feature], the five reference counters per sample, the five verdict counters
//                  (<false>: the barcode table read from global memory; <true>: copied into LDS when the kernel starts)
// The per-lane logic (DemuxDev, demux_find, demux_decide, DemuxHook) lives in f2q_device.h, the table builder
// (demux_validate, demux_build) in f2q_host.h.
#pragma once

// which instance a context launches unless F2Q_DEMUX_TABLE says otherwise.  From the A/B run of scripts/demux_rates.py
// (profiles/r14_demux_rates.txt): the LDS copy was 2 % to 9 % slower where it applies, so global memory it is
#define F2Q_DEMUX_TABLE_LDS_DEFAULT false

// one record: the barcode verdict first (sample = the matrix row), then the routine with the hook that counts into that
// row; the read's five reference counters go to st[] as always and once more to its sample's row of the LDS counters
template <class P, class T>
__device__ __forceinline__ void demux_read(const RunDev &run, const LibDev &lib, const EcDev &ec, const Accum &acc, const DemuxDev &dm, T tab,
                                           P seq, int r, P qual, int qn, unsigned long long gi, unsigned long long st[5],
                                           unsigned long long vst[5], uint32_t *ss)
{
    uint32_t sample = dm.n;
    const int v = demux_decide(dm, tab, run.thr, seq, r, qual, qn, sample);
#pragma unroll
    for (int k = 0; k < 5; k++) vst[k] += (unsigned long long)(v == k);
    const DemuxHook hook{dm.matrix + (unsigned long long)sample * dm.n_features};
    unsigned long long one[5] = {0, 0, 0, 0, 0};
    general_read<P, true, false>(run, lib, ec, acc, seq, r, qual, qn, gi, one, nullptr, 0, 0, hook);
#pragma unroll
    for (int k = 0; k < 5; k++) {
        st[k] += one[k];
        if (one[k]) atomicAdd(&ss[sample * 5u + (uint32_t)k], (uint32_t)one[k]);      // (the routine adds at most 1 per counter and read)
    }
}

// k_count_umi's shape: 64-thread workgroups, the record's two lines staged in LDS, a record longer than the staging area
// walked in global memory.  Single-end Counter mode only (f2q_set_sample_barcodes refuses everything else).
// Dynamic LDS, after the staging area: [LDS_TABLE: the table, dm.mask + 1 slots of 8 bytes, at most 32 KiB]
// [(dm.n + 1) * 5 u32 counters, at most 20 500 bytes].  A u32 counter holds the reads of ONE workgroup of ONE launch
// (a block has fewer than 2^32 records), so it cannot wrap; the non-zero ones are added to dm.sstats when the kernel ends.
template <bool LDS_TABLE>
__global__ __launch_bounds__(F2Q_GEN_THREADS) void k_count_demux(const RunDev *__restrict__ runp, const LibDev *__restrict__ libp,
                                                                  EcDev ec, RawBlock rb, Accum acc, DemuxDev dm)
{
    __shared__ uint32_t stage[F2Q_GEN_THREADS * F2Q_GEN_STRIDE];
    extern __shared__ unsigned long long demux_smem[];
    const RunDev &run = *runp;
    const LibDev &lib = *libp;
    const uint32_t n_slots = LDS_TABLE ? dm.mask + 1u : 0u, n_ss = (dm.n + 1u) * 5u;
    uint32_t *ss = reinterpret_cast<uint32_t *>(demux_smem + n_slots);
    for (uint32_t i = threadIdx.x; i < n_ss; i += F2Q_GEN_THREADS) ss[i] = 0u;
    if (LDS_TABLE) for (uint32_t i = threadIdx.x; i < n_slots; i += F2Q_GEN_THREADS) demux_smem[i] = gp(dm.table)[i];
    __syncthreads();
    unsigned long long st[5] = {0, 0, 0, 0, 0};
    unsigned long long vst[5] = {0, 0, 0, 0, 0};
    const auto raw = gp(rb.raw);
    uint32_t *mine = stage + threadIdx.x * F2Q_GEN_STRIDE;
    for (uint64_t i = (uint64_t)blockIdx.x * F2Q_GEN_THREADS + threadIdx.x; i < rb.n; i += (uint64_t)gridDim.x * F2Q_GEN_THREADS) {
        const unsigned long long so = gp(rb.off)[i];
        const int r = (int)gp(rb.len)[i], qn = (int)gp(rb.qlen)[i];
        const unsigned long long qo = rb.qoff ? gp(rb.qoff)[i] : so + (unsigned long long)r;
        const unsigned long long gi = rb.first_index + (rb.index ? gp(rb.index)[i] : i);
        const uint32_t ms = (uint32_t)so & 3u, mq = (uint32_t)qo & 3u;
        if (r >= 0 && qn >= 0 && ms + (uint32_t)r <= 4u * F2Q_GEN_WORDS && mq + (uint32_t)qn <= 4u * F2Q_GEN_WORDS) {
            stage_line(mine, raw, so, r);
            stage_line(mine + F2Q_GEN_WORDS, raw, qo, qn);
            const uint8_t *sl = reinterpret_cast<const uint8_t *>(mine) + ms;
            const uint8_t *ql = reinterpret_cast<const uint8_t *>(mine + F2Q_GEN_WORDS) + mq;
            if constexpr (LDS_TABLE) demux_read<const uint8_t *>(run, lib, ec, acc, dm, (const unsigned long long *)demux_smem, sl, r, ql, qn, gi, st, vst, ss);
            else demux_read<const uint8_t *>(run, lib, ec, acc, dm, gp(dm.table), sl, r, ql, qn, gi, st, vst, ss);
        } else if constexpr (LDS_TABLE) demux_read<gbytes>(run, lib, ec, acc, dm, (const unsigned long long *)demux_smem, raw + so, r, raw + qo, qn, gi, st, vst, ss);
        else demux_read<gbytes>(run, lib, ec, acc, dm, gp(dm.table), raw + so, r, raw + qo, qn, gi, st, vst, ss);
    }
    // one wave per workgroup: at most one atomic per verdict counter
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const unsigned long long v = wave_sum(vst[k]);
        if (threadIdx.x == 0 && v) acc_add(&dm.verdicts[k], v);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_ss; i += F2Q_GEN_THREADS) {
        const uint32_t v = ss[i];
        if (v) acc_add(&dm.sstats[i], (unsigned long long)v);
    }
    __shared__ unsigned long long st_lds[8];
    flush_stats(acc, st, st_lds, nullptr);
}
