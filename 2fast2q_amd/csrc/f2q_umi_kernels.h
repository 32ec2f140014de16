// f2q_umi_kernels.h -- distinct UMIs per feature (--umi, f2q_set_umi; included by f2q_lib.hip only).
//   k_count_umi    Counter mode on raw records, the byte-exact routine, plus the (feature, UMI) set: one pass
//   k_umi_rehash   the pairs of a full set into a larger one
// The per-lane logic (UmiDev, umi_insert, umi_codes, UmiHook) lives in f2q_device.h.
#pragma once

// k_count_general's shape (64-thread workgroups, the record's two lines staged in LDS, a record longer than the staging
// area walked in global memory); a read the routine assigns to a feature also brings its UMI to the set.  Single-end
// Counter mode only (f2q_set_umi refuses everything else).  The host has sized the set so that every record of the
// launch could bring a new pair and it would still be at most half full.
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
        const uint32_t ms = (uint32_t)so & 3u, mq = (uint32_t)qo & 3u;
        if (r >= 0 && qn >= 0 && ms + (uint32_t)r <= 4u * F2Q_GEN_WORDS && mq + (uint32_t)qn <= 4u * F2Q_GEN_WORDS) {
            stage_line(mine, raw, so, r);
            stage_line(mine + F2Q_GEN_WORDS, raw, qo, qn);
            const uint8_t *sl = reinterpret_cast<const uint8_t *>(mine) + ms;
            const uint8_t *ql = reinterpret_cast<const uint8_t *>(mine + F2Q_GEN_WORDS) + mq;
            const UmiHook<const uint8_t *> hook{&umi, run.thr, sl, r, ql, qn, ust};
            general_read<const uint8_t *, true, false>(run, lib, ec, acc, sl, r, ql, qn, gi, st, nullptr, 0, 0, hook);
        } else {
            const UmiHook<gbytes> hook{&umi, run.thr, raw + so, r, raw + qo, qn, ust};
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

// every pair of `old` into `nw` (empty, with room for them all); umis[] and the counters are shared and stay as they are
__global__ __launch_bounds__(256) void k_umi_rehash(UmiDev old, UmiDev nw)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > old.mask) return;
    const unsigned long long k = gp(old.slots)[i];
    if (k != KEY_EMPTY) (void)umi_claim(nw, k);
}
