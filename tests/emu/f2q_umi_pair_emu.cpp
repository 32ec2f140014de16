// tests/emu/f2q_umi_pair_emu.cpp -- TEST INFRASTRUCTURE.  The host twin of k_count_umi_pair: the paired emulation
// (f2q_pair_emu.cpp, included whole: frame_fastq twice + pack_pairs) with the plan of a paired UMI context -- no fast
// path, so every pair becomes a merged raw record, as f2q_set_umi_paired leaves it -- and then, record by record, what a
// lane of the kernel does: general_read<.., PAIRED> with a UmiPairHook (umi_codes_paired / umi_insert / umi_claim of
// 2fast2q_amd/csrc/f2q_device.h) over a set sized by pairset_reserve's rule (at most half full after a block in which every
// pair is new; growth is umi_rehash_one over every slot).  The product never uses this file.
// -DF2Q_UMI_PAIR_EMU_MAIN: a stand-alone program over a built-in sample (for -fsanitize=address,undefined builds).
#include <stdio.h>

#include <algorithm>

#include "f2q_pair_emu.cpp"

struct UPEmu {
    PEmu *e = nullptr;
    UmiDev u{};
    std::vector<unsigned long long> slots, umis, ctr;
    std::vector<uint32_t> reads;
    bool keep_reads = false;
    uint64_t min_slots = 1u << 16, rehashes = 0;
};

static void upemu_bind(UPEmu *x)
{
    x->umis.assign(std::max<size_t>(x->e->ix.n_features, 1), 0ull);
    x->ctr.assign(F2Q_UMI_CTR_WORDS, 0ull);
    x->slots.clear(); x->reads.clear();
    x->u.slots = nullptr; x->u.reads = nullptr; x->u.mask = 0; x->u.umis = x->umis.data(); x->u.ctr = x->ctr.data();
}

// room for n more pairs at a load of at most one half
static void upemu_reserve(UPEmu *x, uint64_t n)
{
    const uint64_t held = x->ctr[F2Q_UMI_HELD];
    if (!x->slots.empty() && 2 * (held + n) <= x->slots.size()) return;
    uint64_t slots = std::max<uint64_t>(x->min_slots, 2);
    while (slots < 2 * (held + n) || slots < 4 * held) slots <<= 1;
    std::vector<unsigned long long> fresh(slots, KEY_EMPTY);
    std::vector<uint32_t> fresh_reads(x->keep_reads ? slots : 0, 0u);
    UmiDev nw = x->u; nw.slots = fresh.data(); nw.reads = x->keep_reads ? fresh_reads.data() : nullptr; nw.mask = (uint32_t)(slots - 1);
    if (held) {
        for (uint32_t i = 0; i < (uint32_t)x->slots.size(); i++) { if (x->keep_reads) umi_rehash_one<true>(x->u, nw, i); else umi_rehash_one<false>(x->u, nw, i); }
        x->rehashes++;
    }
    x->slots.swap(fresh); x->reads.swap(fresh_reads);
    x->u.slots = x->slots.data(); x->u.reads = x->keep_reads ? x->reads.data() : nullptr; x->u.mask = nw.mask;
}

// the merged records of the packed block through the byte-exact routine with the paired hook
template <bool READS>
static void upemu_walk(UPEmu *x)
{
    PEmu *e = x->e;
    const HostPacked &hp = e->hp;
    Accum acc{e->acc.data(), e->acc.data() + e->ix.n_features, nullptr, nullptr, nullptr, nullptr};
    for (size_t g = 0; g < hp.g_len.size(); g++) {
        const uint8_t *seq = hp.raw.data() + hp.g_off[g], *qual = seq + hp.g_len[g];
        const int r = (int)hp.g_len[g], qn = (int)hp.g_qlen[g], r1 = (int)hp.g_len1[g], qn1 = (int)hp.g_qlen1[g];
        unsigned long long ust[3] = {0, 0, 0};
        const UmiPairHook<const uint8_t *, READS> hook{&x->u, e->run.thr, seq, r, r1, qual, qn, qn1, ust};
        general_read<const uint8_t *, true, true>(e->run, e->lib, e->ec, acc, seq, r, qual, qn, e->reads_seen + hp.g_index[g], acc.stats, nullptr, r1, qn1, hook);
        x->ctr[F2Q_UMI_READS] += ust[0]; x->ctr[F2Q_UMI_FAILED] += ust[1]; x->ctr[F2Q_UMI_HELD] += ust[2];
    }
    e->reads_seen += hp.g_len.size();
}

extern "C" {

// p->start: the windows of mate 1, then those of mate 2 (pemu_create); the parts as f2q_set_umi_paired takes them
void *upemu_create(const f2q_params *p, int n_mate1, int rc2, int32_t start1, int32_t length1, int32_t start2, int32_t length2,
                   uint64_t min_slots, int keep_reads)
{
    if (p->mode != 0 || n_mate1 < 1 || start1 < 0 || start2 < 0 || length1 < 0 || length2 < 0 || length1 + length2 < 1 ||
        length1 + length2 > F2Q_UMI_MAXLEN) return nullptr;
    PEmu *e = (PEmu *)pemu_create(p, n_mate1, rc2);
    if (!e) return nullptr;
    UPEmu *x = new UPEmu();
    x->e = e; x->keep_reads = keep_reads != 0;
    x->u.length = length1 + length2;
    x->u.start1 = length1 ? start1 : 0; x->u.len1 = length1; x->u.start2 = length2 ? start2 : 0; x->u.len2 = length2; x->u.rc2 = rc2 ? 1 : 0;
    if (min_slots) { x->min_slots = 2; while (x->min_slots < min_slots) x->min_slots <<= 1; }
    upemu_bind(x);
    return x;
}
void upemu_destroy(void *h) { UPEmu *x = (UPEmu *)h; pemu_destroy(x->e); delete x; }

// f2q_set_features on a UMI context: the fast-path flags stay cleared
static void upemu_no_fast_path(PEmu *e)
{
    e->plan.fast_fixed = false; e->plan.fast_anchor = false; e->plan.multi = false; e->plan.multi_pair = false;
    e->plan.inband_n = false; e->plan.n_only = false;
}
void upemu_set_features(void *h, const char *seqs, const uint32_t *offs, uint32_t n)
{
    UPEmu *x = (UPEmu *)h;
    pemu_set_features(x->e, seqs, offs, n);
    upemu_no_fast_path(x->e);
    upemu_bind(x);
}

// one block of pairs; returns the pairs counted, or ~0 when a pair did not become a merged raw record
uint64_t upemu_count_block(void *h, const uint8_t *fq1, size_t n1, const uint8_t *fq2, size_t n2)
{
    UPEmu *x = (UPEmu *)h;
    const uint64_t n = pemu_pack(x->e, fq1, n1, fq2, n2);
    const HostPacked &hp = x->e->hp;
    if (hp.n_clean || hp.g_len.size() != n || hp.g_len1.size() != n) return ~0ull;
    upemu_reserve(x, n);
    if (x->keep_reads) upemu_walk<true>(x); else upemu_walk<false>(x);
    return n;
}

// counts[n], stats[5], umis[n], extra[2]; returns the rehashes so far, -1 when the overflow flag is set
long long upemu_read(void *h, int64_t *counts, int64_t *stats, int64_t *umis, int64_t *extra)
{
    UPEmu *x = (UPEmu *)h;
    pemu_read_counts(x->e, counts, stats);
    for (uint32_t f = 0; f < x->e->ix.n_features; f++) umis[f] = (int64_t)x->umis[f];
    extra[0] = (int64_t)x->ctr[F2Q_UMI_READS]; extra[1] = (int64_t)x->ctr[F2Q_UMI_FAILED];
    return x->ctr[F2Q_UMI_OVERFLOW] ? -1 : (long long)x->rehashes;
}
// the occupied slots in slot order: word = (feature << 32) | codes, reads (0 when not kept); returns how many there are
uint64_t upemu_pairs(void *h, uint64_t cap, uint64_t *words, uint32_t *reads, uint64_t *held, uint64_t *slots)
{
    UPEmu *x = (UPEmu *)h;
    uint64_t n = 0;
    for (size_t i = 0; i < x->slots.size(); i++) {
        if (x->slots[i] == KEY_EMPTY) continue;
        if (n < cap) { words[n] = x->slots[i]; reads[n] = x->keep_reads ? x->reads[i] : 0u; }
        n++;
    }
    *held = x->ctr[F2Q_UMI_HELD]; *slots = x->slots.size();
    return n;
}

void upemu_reset(void *h)
{
    UPEmu *x = (UPEmu *)h;
    std::fill(x->e->acc.begin(), x->e->acc.end(), 0ull);
    x->e->reads_seen = 0;
    std::fill(x->slots.begin(), x->slots.end(), KEY_EMPTY);
    std::fill(x->reads.begin(), x->reads.end(), 0u);
    std::fill(x->umis.begin(), x->umis.end(), 0ull);
    std::fill(x->ctr.begin(), x->ctr.end(), 0ull);
}

}

#ifdef F2Q_UMI_PAIR_EMU_MAIN
// 40 features of 10 + 10 bases (--st 5 / --st2 0), UMI parts 20,6 in mate 1 and 12,10 in mate 2, rc2 on, 3 000 pairs in
// blocks of 100 from a set of 64 slots, mates cut short and dirtied at random: the set's own books must agree
int main()
{
    uint64_t z = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { z ^= z << 13; z ^= z >> 7; z ^= z << 17; return z; };
    const int NG = 40, PL = 10, ML = 40;
    std::string seqs; std::vector<uint32_t> offs(1, 0);
    for (int g = 0; g < NG; g++) {
        for (int j = 0; j < 2 * PL + 1; j++) seqs += j == PL ? ':' : "ACGT"[rnd() & 3];
        offs.push_back((uint32_t)seqs.size());
    }
    f2q_params p; memset(&p, 0, sizeof p);
    p.mode = 0; p.miss = 1; p.phred = 30; p.length = PL; p.n_start = 2; p.start[0] = 5; p.start[1] = 0; p.qual_up = p.qual_down = 30;
    void *h = upemu_create(&p, 1, 1, 20, 6, 12, 10, 64, 1);
    if (!h) return 2;
    upemu_set_features(h, seqs.data(), offs.data(), NG);
    auto rc = [](std::string s) { std::reverse(s.begin(), s.end()); for (char &c : s) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c; return s; };
    for (int b = 0; b < 30; b++) {
        std::string fq1, fq2;
        for (int i = 0; i < 100; i++) {
            const size_t g = (size_t)(rnd() % NG) * (2 * PL + 1);
            std::string s1, taken;                                   // taken: mate 2 as the run takes it
            for (int j = 0; j < ML; j++) { s1 += "ACGT"[rnd() & 3]; taken += "ACGT"[rnd() & 3]; }
            s1.replace(5, PL, seqs.substr(g, PL)); taken.replace(0, PL, seqs.substr(g + PL + 1, PL));
            std::string s2 = rc(taken), q1(ML, 'I'), q2(ML, 'I');
            if (rnd() % 10 == 0) s2[12 + rnd() % 10] = 'N';
            if (rnd() % 10 == 0) q2[12 + rnd() % 10] = '#';
            if (rnd() % 10 == 0) q1[20 + rnd() % 6] = '#';
            if (rnd() % 10 == 0) { s2.resize(12 + rnd() % 12); q2.resize(s2.size()); }
            if (rnd() % 10 == 0) q2.resize(rnd() % q2.size());
            if (rnd() % 20 == 0) { s1.resize(rnd() % ML); q1.resize(s1.size()); }
            fq1 += "@a\n" + s1 + "\n+\n" + q1 + "\n"; fq2 += "@b\n" + s2 + "\n+\n" + q2 + "\n";
        }
        if (upemu_count_block(h, (const uint8_t *)fq1.data(), fq1.size(), (const uint8_t *)fq2.data(), fq2.size()) != 100) return 3;
    }
    std::vector<int64_t> counts(NG), umis(NG); int64_t stats[5], extra[2];
    const long long rehashes = upemu_read(h, counts.data(), stats, umis.data(), extra);
    std::vector<uint64_t> words(4096); std::vector<uint32_t> reads(4096); uint64_t held, slots;
    const uint64_t occupied = upemu_pairs(h, words.size(), words.data(), reads.data(), &held, &slots);
    int64_t sum = 0, kept = 0;
    for (int64_t v : umis) sum += v;
    for (uint64_t i = 0; i < occupied && i < reads.size(); i++) kept += reads[i];
    printf("pairs %lld assigned %lld umi_reads %lld umi_failed %lld set %lld slots %llu rehashes %lld\n", (long long)stats[0],
           (long long)(stats[1] + stats[2]), (long long)extra[0], (long long)extra[1], (long long)sum, (unsigned long long)slots, rehashes);
    const bool ok = rehashes >= 3 && stats[0] == 3000 && extra[0] + extra[1] == stats[1] + stats[2] && extra[0] > 0 && extra[1] > 0 &&
                    (uint64_t)sum == held && held == occupied && 2 * held <= slots && kept == extra[0];
    upemu_destroy(h);
    return ok ? 0 : 1;
}
#endif
