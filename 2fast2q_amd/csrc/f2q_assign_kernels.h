// f2q_assign_kernels.h -- Extract+Count with a library: every distinct key of the Extract+Count tables is matched once
// against the assign library (f2q_ec_assign; included by f2q_lib.hip only).
//   k_assign_entries  one lane per entry of the byte-string table
//   k_assign_slots    one lane per slot of the single-word table
// The per-key logic is assign_entry_lane / assign_slot_lane (f2q_device.h), which end in match_key's verdict.  Both
// kernels only READ the tables: they run on the context's stream after every counting launch, deferred pass and
// hot-key flush of the calls before (the hot-key kernels add their LDS counters to the table when a workgroup ends, so
// the counts are complete once the launch is), and after the raw records' stream has been joined.
#pragma once

#define F2Q_ASG_THREADS 256

// st[1..3]: reads per verdict of this lane's keys, summed per wave, then per workgroup: one atomic per stat and workgroup
__device__ __forceinline__ void assign_flush(unsigned long long *stats, unsigned long long st[5])
{
    __shared__ unsigned long long st_lds[8];
    Accum acc{nullptr, stats, nullptr, nullptr, nullptr, nullptr};
    flush_stats(acc, st, st_lds, nullptr);
}

__global__ __launch_bounds__(F2Q_ASG_THREADS) void k_assign_entries(const RunDev *__restrict__ runp, const LibDev *__restrict__ libp, EcDev ec,
                                                                     AssignDev out, unsigned long long n_entries, unsigned long long arena_used,
                                                                     unsigned long long *stats)
{
    const RunDev &run = *runp;
    const LibDev &lib = *libp;
    unsigned long long st[5] = {0, 0, 0, 0, 0};
    for (unsigned long long e = (unsigned long long)blockIdx.x * F2Q_ASG_THREADS + threadIdx.x; e < n_entries;
         e += (unsigned long long)gridDim.x * F2Q_ASG_THREADS) {
        unsigned long long n = 0;
        const int res = assign_entry_lane(run, lib, ec, out, e, arena_used, n);
        st[1] += res == 1 ? n : 0ull; st[2] += res == 2 ? n : 0ull; st[3] += res == 3 ? n : 0ull;
    }
    assign_flush(stats, st);
}

__global__ __launch_bounds__(F2Q_ASG_THREADS) void k_assign_slots(const RunDev *__restrict__ runp, const LibDev *__restrict__ libp, EcDev ec,
                                                                   AssignDev out, unsigned long long *stats)
{
    const RunDev &run = *runp;
    const LibDev &lib = *libp;
    unsigned long long st[5] = {0, 0, 0, 0, 0};
    const unsigned long long n_slots = (unsigned long long)ec.k64_mask + 1ull;
    for (unsigned long long s = (unsigned long long)blockIdx.x * F2Q_ASG_THREADS + threadIdx.x; s < n_slots;
         s += (unsigned long long)gridDim.x * F2Q_ASG_THREADS) {
        unsigned long long n = 0;
        const int res = assign_slot_lane(run, lib, ec, out, (uint32_t)s, n);
        st[1] += res == 1 ? n : 0ull; st[2] += res == 2 ? n : 0ull; st[3] += res == 3 ? n : 0ull;
    }
    assign_flush(stats, st);
}
