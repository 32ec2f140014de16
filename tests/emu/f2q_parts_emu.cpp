// tests/emu/f2q_parts_emu.cpp -- TEST INFRASTRUCTURE.  The host twin of k_count_parts<false / true>: the paired emulation
// (f2q_pair_emu.cpp, included whole: frame_fastq + pack_records / pack_pairs) with the plan of a parts context -- no fast
// path, so every read or pair becomes a raw record, as f2q_set_parts leaves it -- and then, record by record, what a lane
// of the kernel does: parts_read (general_read for the joined verdict, part_verdict twice, parts_class, the pair table, the
// recombinant set through umi_claim_at / umi_read_add) of 2fast2q_amd/csrc/f2q_device.h, over tables built by
// parts_validate / parts_build of f2q_host.h and a set sized by pairset_reserve's rule (growth is umi_rehash_one<true> over
// every slot).  The product never uses this file.
// -DF2Q_PARTS_EMU_MAIN: a stand-alone program over a built-in sample (for -fsanitize=address,undefined builds).
#include <stdio.h>

#include <algorithm>

#include "f2q_pair_emu.cpp"

struct PtEmu {
    PEmu *e = nullptr;                       // null: tables alone (ptemu_table)
    PartsTable tab;
    HostIndex ix[2];
    LibDev lib[2];
    PartsDev d{};
    std::vector<unsigned long long> words, ctr, slots;
    std::vector<uint32_t> reads;
    uint64_t min_slots = 1u << 16, rehashes = 0;
};

static void view_lib(const HostIndex &ix, LibDev &L)
{
    memset(&L, 0, sizeof L);
    L.n_features = ix.n_features; L.n_irregular = ix.n_irregular;
    L.tab_keys = ix.tab_keys.data(); L.tab_idx = ix.tab_idx.data();
    L.ptab = ix.ptab.data(); L.pk = ix.pk;
    memcpy(L.mpk, ix.mpk, sizeof L.mpk); L.mw_ok = ix.mw_ok;
    L.feat_bytes = ix.feat_bytes.data(); L.feat_off = ix.feat_off.data(); L.irr_ids = ix.irr_ids.data();
    L.lt = ix.lt; L.lt.tags = ix.lt_tags.data(); L.lt.slot_of = ix.lt_slot_of.data(); L.lt.feat_of = ix.lt_feat_of.data();
    L.pw = ix.pw; L.pw.tab = ix.pw_tab.data();
    L.pt = ix.pt; L.pt.tags0 = ix.pt_tags0.data(); L.pt.tags1 = ix.pt_tags1.data(); L.pt.pstart = ix.pt_pstart.data();
    L.pt.slot0_of = ix.pt_slot0_of.data(); L.pt.slot1_of = ix.pt_slot1_of.data(); L.pt.feat_of = ix.pt_feat_of.data();
    L.pt.feat0_of = ix.pt_feat0_of.data();
    L.gk.n_groups = ix.n_features ? (uint32_t)ix.gk_groups.size() : 0u; L.gk.grp = ix.gk_groups.data();
    L.gk.tab = ix.gk_tab.data(); L.gk.ids = ix.gk_ids.data();
    L.gk.fw = ix.gk_fw.data(); L.gk.fwoff = ix.gk_fwoff.data();
    memcpy(L.grp, ix.grp, sizeof L.grp);
}

// what parts_install does with a library: F2Q_OK, or F2Q_EINVAL with the message in err (the emulator is left as it was)
static int ptemu_install(PtEmu *x, const char *seqs, const uint32_t *offs, uint32_t n, int miss, std::string &err)
{
    PartsTable t;
    if (int rc = parts_validate(seqs, offs, n, t, err)) return rc;
    parts_build(t);
    x->tab = std::move(t);
    const uint64_t nf = std::max<uint64_t>(n, 1), n1 = std::max<uint64_t>(x->tab.n(0), 1), n2 = std::max<uint64_t>(x->tab.n(1), 1);
    for (int k = 0; k < 2; k++) {
        build_index(x->ix[k], x->tab.seqs[k].data(), x->tab.offs[k].data(), x->tab.n(k), miss, 0);
        view_lib(x->ix[k], x->lib[k]);
    }
    x->words.assign(nf + n1 + n2 + F2Q_PARTS_CLASSES, 0ull); x->ctr.assign(F2Q_UMI_CTR_WORDS, 0ull);
    x->slots.clear(); x->reads.clear();
    PartsDev &d = x->d;
    d = PartsDev{};
    d.lib1 = &x->lib[0]; d.lib2 = &x->lib[1]; d.pair_keys = x->tab.keys.data(); d.pair_feat = x->tab.feat.data(); d.pair_mask = x->tab.mask;
    d.n_features = n; d.ids = x->tab.ids.data();
    d.counts = x->words.data(); d.part1 = d.counts + nf; d.part2 = d.part1 + n1; d.classes = d.part2 + n2;
    d.rec.ctr = x->ctr.data();
    return F2Q_OK;
}

// room for n more pairs at a load of at most one half (pairset_reserve)
static void ptemu_reserve(PtEmu *x, uint64_t n)
{
    const uint64_t held = x->ctr[F2Q_UMI_HELD];
    if (!x->slots.empty() && 2 * (held + n) <= x->slots.size()) return;
    uint64_t slots = std::max<uint64_t>(x->min_slots, 2);
    while (slots < 2 * (held + n) || slots < 4 * held) slots <<= 1;
    std::vector<unsigned long long> fresh(slots, KEY_EMPTY);
    std::vector<uint32_t> fresh_reads(slots, 0u);
    UmiDev nw = x->d.rec; nw.slots = fresh.data(); nw.reads = fresh_reads.data(); nw.mask = (uint32_t)(slots - 1);
    if (held) {
        for (uint32_t i = 0; i < (uint32_t)x->slots.size(); i++) umi_rehash_one<true>(x->d.rec, nw, i);
        x->rehashes++;
    }
    x->slots.swap(fresh); x->reads.swap(fresh_reads);
    x->d.rec.slots = x->slots.data(); x->d.rec.reads = x->reads.data(); x->d.rec.mask = nw.mask;
}

template <bool PAIRED>
static void ptemu_walk(PtEmu *x)
{
    PEmu *e = x->e;
    const HostPacked &hp = e->hp;
    Accum acc{e->acc.data(), e->acc.data() + e->ix.n_features, nullptr, nullptr, nullptr, nullptr};
    for (size_t g = 0; g < hp.g_len.size(); g++) {
        const uint8_t *seq = hp.raw.data() + hp.g_off[g], *qual = seq + hp.g_len[g];
        unsigned long long cst[F2Q_PARTS_CLASSES + 1] = {0, 0, 0, 0, 0, 0, 0};
        parts_read<const uint8_t *, PAIRED>(e->run, e->lib, e->ec, acc, x->d, seq, (int)hp.g_len[g], qual, (int)hp.g_qlen[g], e->reads_seen + hp.g_index[g],
                                            acc.stats, cst, PAIRED ? (int)hp.g_len1[g] : 0, PAIRED ? (int)hp.g_qlen1[g] : 0);
        for (int k = 0; k < F2Q_PARTS_CLASSES; k++) x->d.classes[k] += cst[k];
        x->ctr[F2Q_UMI_HELD] += cst[F2Q_PARTS_CLASSES];
    }
    e->reads_seen += hp.g_len.size();
}

extern "C" {

// f2q_set_parts' library check: the F2Q_E* code, the message in msg
int ptemu_validate(const char *seqs, const uint32_t *offs, uint32_t n, char *msg, size_t cap)
{
    PartsTable t; std::string err;
    const int rc = parts_validate(seqs, offs, n, t, err);
    if (msg && cap) { strncpy(msg, err.c_str(), cap - 1); msg[cap - 1] = 0; }
    return rc;
}

// tables alone
void *ptemu_table(const char *seqs, const uint32_t *offs, uint32_t n)
{
    PtEmu *x = new PtEmu();
    std::string err;
    if (ptemu_install(x, seqs, offs, n, 0, err)) { delete x; return nullptr; }
    return x;
}
void ptemu_info(void *h, uint32_t *n1, uint32_t *n2, uint64_t *slots, uint32_t *pairs)
{
    PtEmu *x = (PtEmu *)h;
    *n1 = x->tab.n(0); *n2 = x->tab.n(1); *slots = x->tab.keys.size(); *pairs = x->tab.pairs;
}
// part i of position pos (0 / 1): its bytes into buf, its length returned
uint32_t ptemu_part(void *h, int pos, uint32_t i, char *buf, size_t cap)
{
    PtEmu *x = (PtEmu *)h;
    const uint32_t a = x->tab.offs[pos][i], b = x->tab.offs[pos][i + 1];
    if (b - a <= cap) memcpy(buf, x->tab.seqs[pos].data() + a, b - a);
    return b - a;
}
// ids[2 * n_features]; the feature the table gives each of those pairs back (F2Q_PARTS_NONE: none)
void ptemu_pairs(void *h, uint32_t *ids, uint32_t *found)
{
    PtEmu *x = (PtEmu *)h;
    for (size_t i = 0; i < x->tab.ids.size(); i++) ids[i] = x->tab.ids[i];
    for (size_t f = 0; f < x->tab.ids.size() / 2; f++) found[f] = parts_pair_find(x->d, x->tab.ids[2 * f], x->tab.ids[2 * f + 1]);
}
uint32_t ptemu_find(void *h, uint32_t i1, uint32_t i2) { return parts_pair_find(((PtEmu *)h)->d, i1, i2); }

// a counting context.  p->start: window 1, window 2 (n_mate1 = 1: window 2 lies in mate 2; 0: single reads)
void *ptemu_create(const f2q_params *p, int n_mate1, int rc2, uint64_t min_slots)
{
    if (p->mode != 0 || p->n_start != 2 || p->n_upstream || p->n_downstream || (n_mate1 != 0 && n_mate1 != 1)) return nullptr;
    PEmu *e = (PEmu *)pemu_create(p, n_mate1, rc2);
    if (!e) return nullptr;
    PtEmu *x = new PtEmu();
    x->e = e;
    if (min_slots) { x->min_slots = 2; while (x->min_slots < min_slots) x->min_slots <<= 1; }
    return x;
}
void ptemu_destroy(void *h) { PtEmu *x = (PtEmu *)h; if (x->e) pemu_destroy(x->e); delete x; }

int ptemu_set_features(void *h, const char *seqs, const uint32_t *offs, uint32_t n, char *msg, size_t cap)
{
    PtEmu *x = (PtEmu *)h;
    std::string err;
    { PartsTable t; if (int rc = parts_validate(seqs, offs, n, t, err)) { if (msg && cap) { strncpy(msg, err.c_str(), cap - 1); msg[cap - 1] = 0; } return rc; } }
    pemu_set_features(x->e, seqs, offs, n);
    PackPlan &pl = x->e->plan;                                    // f2q_set_parts: the fast-path flags stay cleared
    pl.fast_fixed = false; pl.fast_anchor = false; pl.multi = false; pl.multi_pair = false; pl.inband_n = false; pl.n_only = false;
    x->rehashes = 0;
    return ptemu_install(x, seqs, offs, n, x->e->run.miss, err);
}

// one block (fq2 == NULL: single reads); returns the records counted, or ~0 when one did not become a raw record
uint64_t ptemu_count_block(void *h, const uint8_t *fq1, size_t n1, const uint8_t *fq2, size_t n2)
{
    PtEmu *x = (PtEmu *)h;
    const uint64_t n = pemu_pack(x->e, fq1, n1, fq2, n2);
    const HostPacked &hp = x->e->hp;
    if (hp.n_clean || hp.g_len.size() != n || (fq2 ? hp.g_len1.size() != n : !hp.g_len1.empty())) return ~0ull;
    ptemu_reserve(x, n);
    if (fq2) ptemu_walk<true>(x); else ptemu_walk<false>(x);
    return n;
}

// counts[nf], stats[5], parts_counts[nf], part1[n1], part2[n2], classes[6]; returns the rehashes so far, -1 when the overflow flag is set
long long ptemu_read(void *h, int64_t *counts, int64_t *stats, int64_t *parts_counts, int64_t *part1, int64_t *part2, int64_t *classes)
{
    PtEmu *x = (PtEmu *)h;
    pemu_read_counts(x->e, counts, stats);
    for (uint32_t f = 0; f < x->e->ix.n_features; f++) parts_counts[f] = (int64_t)x->d.counts[f];
    for (uint32_t i = 0; i < x->tab.n(0); i++) part1[i] = (int64_t)x->d.part1[i];
    for (uint32_t i = 0; i < x->tab.n(1); i++) part2[i] = (int64_t)x->d.part2[i];
    for (int k = 0; k < F2Q_PARTS_CLASSES; k++) classes[k] = (int64_t)x->d.classes[k];
    return x->ctr[F2Q_UMI_OVERFLOW] ? -1 : (long long)x->rehashes;
}
// the recombinant pairs sorted by (i1, i2), as f2q_parts_recombinants; returns how many there are; *held = the set's counter
uint64_t ptemu_recombinants(void *h, uint64_t cap, uint32_t *i1, uint32_t *i2, uint32_t *reads, uint64_t *held, uint64_t *slots)
{
    PtEmu *x = (PtEmu *)h;
    std::vector<std::pair<unsigned long long, uint32_t>> v;
    for (size_t i = 0; i < x->slots.size(); i++) if (x->slots[i] != KEY_EMPTY) v.emplace_back(x->slots[i], x->reads[i]);
    std::sort(v.begin(), v.end());
    for (size_t i = 0; i < v.size() && i < cap; i++) { i1[i] = (uint32_t)(v[i].first >> 32); i2[i] = (uint32_t)v[i].first; reads[i] = v[i].second; }
    *held = x->ctr[F2Q_UMI_HELD]; *slots = x->slots.size();
    return v.size();
}

void ptemu_reset(void *h)
{
    PtEmu *x = (PtEmu *)h;
    std::fill(x->e->acc.begin(), x->e->acc.end(), 0ull);
    x->e->reads_seen = 0;
    std::fill(x->words.begin(), x->words.end(), 0ull);
    std::fill(x->ctr.begin(), x->ctr.end(), 0ull);
    std::fill(x->slots.begin(), x->slots.end(), KEY_EMPTY);
    std::fill(x->reads.begin(), x->reads.end(), 0u);
}

}

#ifdef F2Q_PARTS_EMU_MAIN
// 12 x 12 parts of 10 bases, 60 of the 144 pairs in the library; 3 000 single reads (--st 0,20) and 3 000 pairs (--st 5 /
// --st2 0, rc2) in blocks of 100 from a set of 64 slots: planted pairs, recombinants, one substitution per part, junk,
// reads cut short and dirtied at random.  The books of the context must agree among themselves.
int main()
{
    uint64_t z = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { z ^= z << 13; z ^= z >> 7; z ^= z << 17; return z; };
    const int NP = 12, PL = 10, ML = 44;
    std::vector<std::string> pa, pb;
    for (int i = 0; i < NP; i++) { std::string a, b; for (int j = 0; j < PL; j++) { a += "ACGT"[rnd() & 3]; b += "ACGT"[rnd() & 3]; } pa.push_back(a); pb.push_back(b); }
    std::string seqs; std::vector<uint32_t> offs(1, 0);
    for (int i = 0; i < NP; i++) for (int j = 0; j < 5; j++) { seqs += pa[i] + ":" + pb[(i + 3 * j) % NP]; offs.push_back((uint32_t)seqs.size()); }
    const uint32_t NF = (uint32_t)offs.size() - 1;
    auto rc = [](std::string s) { std::reverse(s.begin(), s.end()); for (char &c : s) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c; return s; };
    bool ok = true;
    for (int paired = 0; paired < 2; paired++) {
        f2q_params p; memset(&p, 0, sizeof p);
        p.mode = 0; p.miss = 1; p.phred = 30; p.length = PL; p.n_start = 2; p.start[0] = paired ? 5 : 0; p.start[1] = paired ? 0 : 20; p.qual_up = p.qual_down = 30;
        void *h = ptemu_create(&p, paired, paired, 64);
        if (!h) return 2;
        char msg[256];
        if (ptemu_set_features(h, seqs.data(), offs.data(), NF, msg, sizeof msg)) return 3;
        for (int b = 0; b < 30; b++) {
            std::string fq1, fq2;
            for (int i = 0; i < 100; i++) {
                std::string a = pa[rnd() % NP], bb = rnd() % 4 ? pb[rnd() % NP] : std::string(PL, 'G');
                if (rnd() % 5 == 0) a[rnd() % PL] = "ACGTN"[rnd() % 5];
                if (rnd() % 5 == 0) bb[rnd() % PL] = "ACGTn"[rnd() % 5];
                std::string s1, s2, q1(ML, 'I'), q2(ML, 'I');
                for (int j = 0; j < ML; j++) { s1 += "ACGT"[rnd() & 3]; s2 += "ACGT"[rnd() & 3]; }
                if (paired) { s1.replace(5, PL, a); s2.replace(0, PL, bb); s2 = rc(s2); }
                else { s1.replace(0, PL, a); s1.replace(20, PL, bb); }
                if (rnd() % 12 == 0) q1[rnd() % ML] = '#';
                if (rnd() % 12 == 0) q2[rnd() % ML] = '#';
                if (rnd() % 12 == 0) { s1.resize(rnd() % ML); q1.resize(s1.size()); }
                if (rnd() % 12 == 0) { s2.resize(rnd() % ML); q2.resize(rnd() % (s2.size() + 1)); }
                fq1 += "@a\n" + s1 + "\n+\n" + q1 + "\n"; fq2 += "@b\n" + s2 + "\n+\n" + q2 + "\n";
            }
            if (ptemu_count_block(h, (const uint8_t *)fq1.data(), fq1.size(), paired ? (const uint8_t *)fq2.data() : nullptr, paired ? fq2.size() : 0) != 100) return 4;
        }
        std::vector<int64_t> counts(NF), pc(NF), m1(NP), m2(NP); int64_t stats[5], cls[6];
        const long long rehashes = ptemu_read(h, counts.data(), stats, pc.data(), m1.data(), m2.data(), cls);
        std::vector<uint32_t> i1(4096), i2(4096), rd(4096); uint64_t held, slots;
        const uint64_t nrec = ptemu_recombinants(h, i1.size(), i1.data(), i2.data(), rd.data(), &held, &slots);
        int64_t s_cls = 0, s_pc = 0, s_m1 = 0, s_m2 = 0, s_rd = 0;
        for (int k = 0; k < 6; k++) s_cls += cls[k];
        for (int64_t v : pc) s_pc += v;
        for (int64_t v : m1) s_m1 += v;
        for (int64_t v : m2) s_m2 += v;
        for (uint64_t i = 0; i < nrec; i++) { s_rd += rd[i]; ok = ok && ptemu_find(h, i1[i], i2[i]) == F2Q_PARTS_NONE; }
        printf("%s: reads %lld classes %lld %lld %lld %lld %lld %lld, %llu recombinant pairs in %llu slots, %lld rehashes\n", paired ? "paired" : "single",
               (long long)stats[0], (long long)cls[0], (long long)cls[1], (long long)cls[2], (long long)cls[3], (long long)cls[4], (long long)cls[5],
               (unsigned long long)nrec, (unsigned long long)slots, rehashes);
        ok = ok && rehashes >= 1 && stats[0] == 3000 && s_cls == 3000 && s_pc == cls[0] + cls[1] && s_rd == cls[2] && nrec == held && 2 * held <= slots &&
             s_m1 == cls[0] + cls[1] + cls[2] + cls[3] && s_m2 == cls[0] + cls[1] + cls[2] + cls[4];
        for (int k = 0; k < 6; k++) ok = ok && cls[k] > 0;
        ptemu_destroy(h);
    }
    return ok ? 0 : 1;
}
#endif
