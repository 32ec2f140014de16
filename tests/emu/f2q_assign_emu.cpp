// tests/emu/f2q_assign_emu.cpp -- TEST INFRASTRUCTURE.  The per-key logic of f2q_ec_assign (assign_entry_lane /
// assign_slot_lane of 2fast2q_amd/csrc/f2q_device.h, what k_assign_entries / k_assign_slots run per lane) compiled with
// g++ and run over the Extract+Count tables that the existing emulation (f2q_emu.cpp, included whole) fills, so the CPU
// suite can check it against the oracle.  The product never uses this file.
#include "f2q_emu.cpp"

extern "C" {

// The tables of emulator h as they are now against the library seqs/offs/n (allowed mismatches: the run's --m).
// counts[n], stats[5] (reads and quality_failed are the emulator's own); feature / dist per key in emu_ec_get's order
// (byte-string entries, then the occupied single-word slots), -1 = none.  Returns the number of keys, -1 on a bad entry.
long long aemu_assign(void *h, const char *seqs, const uint32_t *offs, uint32_t n, int64_t *counts, int64_t *stats,
                      int32_t *feature, int32_t *dist)
{
    Emu *e = (Emu *)h;
    Emu lib_only;                                             // (bind_lib wants an Emu: only ix / lib are used)
    lib_only.run = e->run;
    build_index(lib_only.ix, seqs, offs, n, e->run.miss);
    bind_lib(&lib_only);
    const size_t nb = (size_t)e->ctr[0], nw = e->k64s.size();
    std::vector<uint32_t> fb(nb + 1), fw(nw + 1);
    std::vector<uint8_t> db(nb + 1), dw(nw + 1);
    std::vector<unsigned long long> acc(n + 1, 0);
    unsigned long long bad = 0, st[5] = {0, 0, 0, 0, 0};
    AssignDev out{fb.data(), db.data(), fw.data(), dw.data(), acc.data(), &bad};
    for (size_t i = 0; i < nb; i++) {
        unsigned long long reads = 0;
        st[assign_entry_lane(e->run, lib_only.lib, e->ec, out, i, e->ctr[1], reads)] += reads;
    }
    for (size_t s = 0; s < nw; s++) {
        unsigned long long reads = 0;
        st[assign_slot_lane(e->run, lib_only.lib, e->ec, out, (uint32_t)s, reads)] += reads;
    }
    if (bad) return -1;
    for (uint32_t f = 0; f < n; f++) counts[f] = (int64_t)acc[f];
    for (int k = 1; k <= 3; k++) stats[k] = (int64_t)st[k];
    stats[0] = (int64_t)e->acc[e->ix.n_features + 0]; stats[4] = (int64_t)e->acc[e->ix.n_features + 4];
    long long o = 0;
    auto put = [&](uint32_t f, uint8_t d) {
        feature[o] = f == F2Q_ASG_NONE ? -1 : (int32_t)f; dist[o] = d == F2Q_ASG_NODIST ? -1 : (int32_t)d; o++;
    };
    for (size_t i = 0; i < nb; i++) put(fb[i], db[i]);
    for (size_t s = 0; s < nw; s++) if (dw[s] != F2Q_ASG_EMPTY) put(fw[s], dw[s]);
    return o;
}

}
