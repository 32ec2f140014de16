// tests/emu/f2q_pair_emu.cpp -- TEST INFRASTRUCTURE.  The paired-end host twin of the product (frame_fastq twice +
// pack_pairs + general_read<.., PAIRED>, all from 2fast2q_amd/csrc) compiled with g++, so that the CPU suite can check
// (a) that a clean pair is laid into exactly the tile slot the merged read gets from the single-end packer -- the
// counting kernels' lane logic on such tiles is what tests/emu/f2q_emu.cpp already emulates -- and (b) the byte-exact
// routine on merged pairs against the oracle.  The product never uses this file.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../2fast2q_amd/csrc/f2q_device.h"
#include "../../2fast2q_amd/csrc/f2q_host.h"

using namespace f2q;

struct PEmu {
    RunDev run; PackPlan plan; HostIndex ix; LibDev lib; bool rc2 = false;
    std::vector<unsigned long long> acc;
    EcDev ec; std::vector<unsigned long long> slots, ent_off, ent_count, ent_first, ctr, k64s, k64c, k64f; std::vector<uint32_t> ent_len, arena;
    uint64_t reads_seen = 0, fast = 0, general = 0;
    HostPacked hp;
    std::string err;
};

static void bind_lib(PEmu *e)
{
    LibDev &L = e->lib;
    memset(&L, 0, sizeof L);
    L.n_features = e->ix.n_features; L.n_irregular = e->ix.n_irregular;
    L.tab_keys = e->ix.tab_keys.data(); L.tab_idx = e->ix.tab_idx.data();
    L.ptab = e->ix.ptab.data(); L.pk = e->ix.pk;
    memcpy(L.mpk, e->ix.mpk, sizeof L.mpk); L.mw_ok = e->ix.mw_ok;
    L.feat_bytes = e->ix.feat_bytes.data(); L.feat_off = e->ix.feat_off.data(); L.irr_ids = e->ix.irr_ids.data();
    L.lt = e->ix.lt; L.lt.tags = e->ix.lt_tags.data(); L.lt.slot_of = e->ix.lt_slot_of.data(); L.lt.feat_of = e->ix.lt_feat_of.data();
    L.pw = e->ix.pw; L.pw.tab = e->ix.pw_tab.data();
    L.pt = e->ix.pt; L.pt.tags0 = e->ix.pt_tags0.data(); L.pt.tags1 = e->ix.pt_tags1.data(); L.pt.pstart = e->ix.pt_pstart.data();
    L.pt.slot0_of = e->ix.pt_slot0_of.data(); L.pt.slot1_of = e->ix.pt_slot1_of.data(); L.pt.feat_of = e->ix.pt_feat_of.data();
    L.pt.feat0_of = e->ix.pt_feat0_of.data();
    L.gk.n_groups = e->ix.n_features ? (uint32_t)e->ix.gk_groups.size() : 0u; L.gk.grp = e->ix.gk_groups.data();
    L.gk.tab = e->ix.gk_tab.data(); L.gk.ids = e->ix.gk_ids.data();
    L.gk.fw = e->ix.gk_fw.data(); L.gk.fwoff = e->ix.gk_fwoff.data();
    memcpy(L.grp, e->ix.grp, sizeof L.grp);
    e->acc.assign(e->ix.n_features + 5, 0);
}

extern "C" {

// p->start holds the windows of mate 1, then those of mate 2; n_mate1 == 0: a single-end run (the merged-read twin)
void *pemu_create(const f2q_params *p, int n_mate1, int rc2)
{
    PEmu *e = new PEmu();
    if (fill_run(*p, e->run, e->err, n_mate1)) { delete e; return nullptr; }
    e->rc2 = rc2 != 0;
    e->plan = make_plan(e->run); e->plan.rc2 = e->rc2;
    uint32_t z = 0;
    build_index(e->ix, "", &z, 0, e->run.miss, 0);
    bind_lib(e);
    const size_t cap = 1 << 16, slots = 1 << 18;
    e->slots.assign(slots, 0); e->ent_off.assign(cap, 0); e->ent_len.assign(cap, 0); e->ent_count.assign(cap, 0);
    e->ent_first.assign(cap, ~0ull); e->arena.assign(1 << 20, 0); e->ctr.assign(4, 0);
    e->ec.slots = e->slots.data(); e->ec.mask = slots - 1; e->ec.max_entries = cap; e->ec.ent_off = e->ent_off.data();
    e->ec.ent_len = e->ent_len.data(); e->ec.ent_count = e->ent_count.data(); e->ec.ent_first = e->ent_first.data();
    e->ec.arena = e->arena.data(); e->ec.arena_words = e->arena.size(); e->ec.ctr = e->ctr.data();
    e->k64s.assign(slots, ~0ull); e->k64c.assign(slots, 0); e->k64f.assign(slots, ~0ull);
    e->ec.k64_slots = e->k64s.data(); e->ec.k64_count = e->k64c.data(); e->ec.k64_first = e->k64f.data(); e->ec.k64_mask = slots - 1;
    return e;
}
void pemu_destroy(void *h) { delete (PEmu *)h; }

// what f2q_set_features decides for a fixed-offset run
void pemu_set_features(void *h, const char *seqs, const uint32_t *offs, uint32_t n)
{
    PEmu *e = (PEmu *)h;
    e->plan = make_plan(e->run); e->plan.rc2 = e->rc2;
    build_index(e->ix, seqs, offs, n, e->run.miss, e->plan.fast_fixed ? e->run.length : 0, e->plan.multi ? e->run.n_iter : 0);
    if (e->plan.multi && (!e->ix.mw_ok || e->ix.n_irregular)) { e->plan.multi = false; e->plan.fast_fixed = false; }
    bind_lib(e);
    e->plan.inband_n = e->plan.fast_fixed && e->ix.n_irregular == 0;
}
void pemu_force_general(void *h) { PEmu *e = (PEmu *)h; e->plan.fast_fixed = false; }
int pemu_plan_multi(void *h) { return ((PEmu *)h)->plan.multi ? 1 : 0; }

// pack: fq2 != NULL pairs (pack_pairs), else single reads (pack_records); the result stays in the emulator
uint64_t pemu_pack(void *h, const uint8_t *fq1, size_t n1, const uint8_t *fq2, size_t n2)
{
    PEmu *e = (PEmu *)h;
    std::vector<Rec> r1, r2;
    frame_fastq(fq1, n1, r1);
    if (fq2) { frame_fastq(fq2, n2, r2); pack_pairs(e->plan, r1, r2, e->hp); return r1.size() < r2.size() ? r1.size() : r2.size(); }
    pack_records(e->plan, r1, e->hp);
    return r1.size();
}
// sizes: tiles, wb, wq, rmax, clean, general
void pemu_packed_info(void *h, uint64_t out[6])
{
    const HostPacked &hp = ((PEmu *)h)->hp;
    out[0] = hp.n_tiles; out[1] = hp.wb; out[2] = hp.wq; out[3] = hp.rmax; out[4] = hp.n_clean; out[5] = hp.g_len.size();
}
void pemu_packed_get(void *h, uint32_t *bases, uint32_t *qual, uint16_t *len, uint32_t *c_index, uint32_t *g_index)
{
    const HostPacked &hp = ((PEmu *)h)->hp;
    if (!hp.bases.empty()) memcpy(bases, hp.bases.data(), hp.bases.size() * 4);
    if (!hp.qual.empty()) memcpy(qual, hp.qual.data(), hp.qual.size() * 4);
    if (!hp.len.empty()) memcpy(len, hp.len.data(), hp.len.size() * 2);
    if (!hp.c_index.empty()) memcpy(c_index, hp.c_index.data(), hp.c_index.size() * 4);
    if (!hp.g_index.empty()) memcpy(g_index, hp.g_index.data(), hp.g_index.size() * 4);
}

// the raw records of the packed block through the byte-exact routine (every pair after pemu_force_general)
void pemu_count_raw(void *h)
{
    PEmu *e = (PEmu *)h;
    const HostPacked &hp = e->hp;
    Accum acc{e->acc.data(), e->acc.data() + e->ix.n_features, nullptr, nullptr, nullptr, nullptr};
    const bool paired = !hp.g_len1.empty();
    for (size_t g = 0; g < hp.g_len.size(); g++) {
        const uint8_t *seq = hp.raw.data() + hp.g_off[g];
        if (paired)
            general_read<const uint8_t *, true, true>(e->run, e->lib, e->ec, acc, seq, (int)hp.g_len[g], seq + hp.g_len[g], (int)hp.g_qlen[g],
                                                      e->reads_seen + hp.g_index[g], acc.stats, nullptr, (int)hp.g_len1[g], (int)hp.g_qlen1[g]);
        else
            general_read<const uint8_t *, true>(e->run, e->lib, e->ec, acc, seq, (int)hp.g_len[g], seq + hp.g_len[g], (int)hp.g_qlen[g],
                                                e->reads_seen + hp.g_index[g], acc.stats);
    }
    e->reads_seen += hp.n_clean + hp.g_len.size();
}
void pemu_read_counts(void *h, int64_t *counts, int64_t *stats)
{
    PEmu *e = (PEmu *)h;
    for (uint32_t i = 0; i < e->ix.n_features; i++) counts[i] = (int64_t)e->acc[i];
    for (int k = 0; k < 5; k++) stats[k] = (int64_t)e->acc[e->ix.n_features + k];
}
// Extract+Count entries: first the byte-string table, then the occupied slots of the single-word table
static std::vector<size_t> k64_live(PEmu *e) { std::vector<size_t> v; for (size_t i = 0; i < e->k64s.size(); i++) if (e->k64s[i] != ~0ull) v.push_back(i); return v; }
uint64_t pemu_ec_n(void *h) { PEmu *e = (PEmu *)h; return e->ctr[0] + k64_live(e).size(); }
void pemu_ec_get(void *h, uint64_t e_, char *key, uint32_t *len, int64_t *count, uint64_t *first)
{
    PEmu *e = (PEmu *)h;
    if (e_ >= e->ctr[0]) {
        const size_t s = k64_live(e)[e_ - e->ctr[0]];
        *len = ec64_text(e->k64s[s], key); *count = (int64_t)e->k64c[s] + 1; *first = e->k64f[s];
        return;
    }
    *len = e->ent_len[e_]; *count = (int64_t)e->ent_count[e_]; *first = e->ent_first[e_];
    memcpy(key, (const uint8_t *)(e->arena.data() + e->ent_off[e_]), *len);
}

}
