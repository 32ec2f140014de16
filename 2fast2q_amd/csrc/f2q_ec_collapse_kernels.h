// f2q_ec_collapse_kernels.h -- Extract+Count without a library: the keys of the single-word table one base apart are
// folded into the neighbour with the most reads (f2q_ec_collapse; included by f2q_lib.hip only).
//   k_ec_parent / k_ec_parent_lane   parent[s] of every slot: the wave-cooperative layout and the lane-per-slot one
//   k_ec_roots                       root[s], cluster[root] += reads, the four counters
// The per-lane logic is ecc_probe / ecc_parent_lane / ecc_root_lane (f2q_device.h).  Both launches only READ the tables:
// they run on the context's stream after every counting launch, deferred pass and hot-key flush of the calls before, and
// after the raw records' stream has been joined (as the assign kernels do).  parent[] is written once per slot by
// k_ec_parent and read by k_ec_roots only, across the kernel boundary: plain stores and loads.
#pragma once

#define F2Q_ECC_THREADS 256

// k_umi_link's layout.  A table is at most 3/4 full and a key has 3L look-ups, each a dependent probe chain of its own.  A
// wave takes 64 consecutive slots, compacts the eligible ones into its row of LDS (the key word, its reads next to it),
// and then takes them 64 / 3L at a time: lane g * 3L + n probes neighbour n of the g-th key of the round.  L is the
// longest key of the 64 slots (anchored runs hold several lengths: a shorter key leaves its last lanes idle).  Past
// 3L = 64 (L >= 22) a round is one key, lane n takes neighbours n and n + 64.  The candidates of a key are reduced over
// its lanes by shuffles that stay inside the group (most reads, then the smallest neighbour number); the group's first
// lane stores the parent.  Every slot that is not compacted is its own parent.  Any grid: waves stride over the table.
__global__ __launch_bounds__(F2Q_ECC_THREADS) void k_ec_parent(EcDev ec, uint32_t *parent, uint32_t ratio)
{
    __shared__ unsigned long long keys[F2Q_ECC_THREADS / 64][64];
    __shared__ unsigned long long cnts[F2Q_ECC_THREADS / 64][64];
    __shared__ uint8_t from[F2Q_ECC_THREADS / 64][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const unsigned long long slots = (unsigned long long)ec.k64_mask + 1ull;
    for (unsigned long long base = ((unsigned long long)blockIdx.x * waves + wave) * 64ull; base < slots; base += (unsigned long long)gridDim.x * waves * 64ull) {
        const bool in = base + lane < slots;
        const unsigned long long k = in ? gp(ec.k64_slots)[base + lane] : KEY_EMPTY;
        const uint32_t len = ecc_length(k);
        const unsigned long long occ = __ballot(len != 0u);
        if (in && !len) gpw(parent)[base + lane] = (uint32_t)(base + lane);
        if (occ == 0ull) continue;
        if (len) {
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(occ >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)occ, 0u));
            keys[wave][rank] = k; from[wave][rank] = (uint8_t)lane;
            cnts[wave][rank] = gp(ec.k64_count)[base + lane] + 1ull;         // (the count word holds n - 1)
        }
        uint32_t lmax = len;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const uint32_t x = __shfl_xor(lmax, o, 64); lmax = x > lmax ? x : lmax; }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const uint32_t cnt = (uint32_t)__popcll(occ);
        const uint32_t per = 3u * lmax, gsz = per < 64u ? per : 64u, groups = 64u / gsz;
        const uint32_t g = lane / gsz, n0 = lane - g * gsz;
        for (uint32_t t = 0; t < cnt; t += groups) {
            const uint32_t q = t + g;
            const bool act = g < groups && q < cnt;
            EccCand best{0ull, 0u, 0u};
            if (act) {
                const unsigned long long kq = keys[wave][q], c = cnts[wave][q];
                const uint32_t own = 3u * ecc_length(kq);
                for (uint32_t n = n0; n < own; n += 64u) ecc_probe(ec, kq, c, ratio, n, best);
            }
            // every lane takes part in the shuffles; a lane only ever takes from a lane of its own group
            unsigned long long br = best.reads, bsn = ((unsigned long long)best.n << 32) | best.slot;
#pragma unroll
            for (uint32_t off = 1; off < 64u; off <<= 1) {
                const unsigned long long orr = __shfl_down(br, off, 64), osn = __shfl_down(bsn, off, 64);
                if (n0 + off < gsz && (orr > br || (orr == br && orr != 0ull && osn < bsn))) { br = orr; bsn = osn; }
            }
            if (act && n0 == 0u) {
                const uint32_t i = (uint32_t)base + from[wave][q];
                gpw(parent)[i] = br ? (uint32_t)bsn : i;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
}

// the plain layout, kept for the comparison and as the tests' cross-check (F2Q_ECC_LINK=lane): a lane per slot
__global__ __launch_bounds__(F2Q_ECC_THREADS) void k_ec_parent_lane(EcDev ec, uint32_t *parent, uint32_t ratio)
{
    const unsigned long long slots = (unsigned long long)ec.k64_mask + 1ull;
    for (unsigned long long s = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; s < slots; s += (unsigned long long)gridDim.x * blockDim.x)
        ecc_parent_lane(ec, parent, ratio, (uint32_t)s);
}

// after k_ec_parent has ended (parent[] is stable).  cluster[slots + F2Q_ECC_*]: the counters, summed per wave (the chain a
// maximum), one atomic per counter and wave
__global__ __launch_bounds__(F2Q_ECC_THREADS) void k_ec_roots(EcDev ec, const uint32_t *parent, uint32_t *root, unsigned long long *cluster)
{
    const unsigned long long slots = (unsigned long long)ec.k64_mask + 1ull;
    unsigned long long tot[F2Q_ECC_CTR_WORDS] = {0, 0, 0, 0};
    for (unsigned long long s = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; s < slots; s += (unsigned long long)gridDim.x * blockDim.x)
        ecc_root_lane(ec, parent, root, cluster, (uint32_t)s, tot);
    const unsigned long long eligible = wave_sum(tot[F2Q_ECC_ELIGIBLE]), absorbed = wave_sum(tot[F2Q_ECC_ABSORBED]),
                             reads = wave_sum(tot[F2Q_ECC_ABSORBED_READS]);
    uint32_t chain = (uint32_t)tot[F2Q_ECC_CHAIN];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint32_t x = __shfl_xor(chain, o, 64); chain = x > chain ? x : chain; }
    if ((threadIdx.x & 63u) == 0) {
        unsigned long long *ctr = cluster + slots;
        if (eligible) acc_add(&ctr[F2Q_ECC_ELIGIBLE], eligible);
        if (absorbed) acc_add(&ctr[F2Q_ECC_ABSORBED], absorbed);
        if (reads) acc_add(&ctr[F2Q_ECC_ABSORBED_READS], reads);
        if (chain) ecc_max(&ctr[F2Q_ECC_CHAIN], (unsigned long long)chain);
    }
}
