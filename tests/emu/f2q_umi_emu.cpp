// tests/emu/f2q_umi_emu.cpp -- TEST INFRASTRUCTURE.  The per-lane logic of k_count_umi (general_read with a UmiHook,
// umi_codes / umi_insert / umi_claim of 2fast2q_amd/csrc/f2q_device.h) compiled with g++ and run record by record over
// the existing emulation (f2q_emu.cpp, included whole), with the host's sizing rule (pairset_reserve of f2q_lib.hip: at most
// half full after a block in which every record brings a new pair; growth is umi_rehash_one over every slot, as in
// k_umi_rehash; with reads kept, reads[] is allocated zeroed with the set and filled by the rehash), so the CPU suite can
// check it against the oracle.  The product never uses this file.
// -DF2Q_UMI_EMU_MAIN: a stand-alone program over a built-in sample (for -fsanitize=address,undefined builds).
#include "f2q_emu.cpp"

struct UEmu {
    Emu *e = nullptr;
    UmiDev u{};
    std::vector<unsigned long long> slots, umis, ctr;
    std::vector<uint32_t> reads;                                     // keep_reads: parallel to slots (k_count_umi<true>)
    bool keep_reads = false;
    uint64_t min_slots = 1u << 16, rehashes = 0;
};

static void uemu_bind(UEmu *x)
{
    x->umis.assign(std::max<size_t>(x->e->ix.n_features, 1), 0ull);
    x->ctr.assign(F2Q_UMI_CTR_WORDS, 0ull);
    x->slots.clear(); x->reads.clear();
    x->u.slots = nullptr; x->u.reads = nullptr; x->u.mask = 0; x->u.umis = x->umis.data(); x->u.ctr = x->ctr.data();
}

// room for n more pairs at a load of at most one half
static void uemu_reserve(UEmu *x, uint64_t n)
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

// every record through the byte-exact routine with the UMI hook (what a lane of k_count_umi<READS> does)
template <bool READS>
static size_t uemu_count(UEmu *x, const uint8_t *buf, size_t n)
{
    Emu *e = x->e;
    std::vector<Rec> recs;
    const size_t used = frame_fastq(buf, n, recs);
    uemu_reserve(x, recs.size());
    Accum acc{e->acc.data(), e->acc.data() + e->ix.n_features, nullptr, nullptr, nullptr, nullptr};
    for (size_t i = 0; i < recs.size(); i++) {
        unsigned long long ust[3] = {0, 0, 0};
        const UmiHook<const uint8_t *, READS> hook{&x->u, e->run.thr, recs[i].seq, (int)recs[i].len, recs[i].qual, (int)recs[i].qlen, ust};
        general_read<const uint8_t *, true, false>(e->run, e->lib, e->ec, acc, recs[i].seq, (int)recs[i].len, recs[i].qual, (int)recs[i].qlen,
                                                   e->reads_seen + i, acc.stats, nullptr, 0, 0, hook);
        x->ctr[F2Q_UMI_READS] += ust[0]; x->ctr[F2Q_UMI_FAILED] += ust[1]; x->ctr[F2Q_UMI_HELD] += ust[2];
    }
    e->reads_seen += recs.size(); e->general += recs.size();
    return used;
}

extern "C" {

void *uemu_create(const f2q_params *p, int32_t start, int32_t length, uint64_t min_slots)
{
    if (p->mode != 0 || start < 0 || length < 1 || length > F2Q_UMI_MAXLEN) return nullptr;
    Emu *e = (Emu *)emu_create(p);
    if (!e) return nullptr;
    UEmu *x = new UEmu();
    x->e = e; x->u.start = start; x->u.length = length;
    if (min_slots) { x->min_slots = 2; while (x->min_slots < min_slots) x->min_slots <<= 1; }
    uemu_bind(x);
    return x;
}
void uemu_destroy(void *h) { UEmu *x = (UEmu *)h; emu_destroy(x->e); delete x; }

void uemu_set_features(void *h, const char *seqs, const uint32_t *offs, uint32_t n)
{
    UEmu *x = (UEmu *)h;
    emu_set_features(x->e, seqs, offs, n);
    uemu_bind(x);
}

size_t uemu_count_block(void *h, const uint8_t *buf, size_t n)
{
    UEmu *x = (UEmu *)h;
    return x->keep_reads ? uemu_count<true>(x, buf, n) : uemu_count<false>(x, buf, n);
}

// counts[n], stats[5], umis[n], extra[2]; returns the rehashes so far, -1 when the overflow flag is set
long long uemu_read(void *h, int64_t *counts, int64_t *stats, int64_t *umis, int64_t *extra)
{
    UEmu *x = (UEmu *)h;
    emu_read_counts(x->e, counts, stats, nullptr, nullptr);
    for (uint32_t f = 0; f < x->e->ix.n_features; f++) umis[f] = (int64_t)x->umis[f];
    extra[0] = (int64_t)x->ctr[F2Q_UMI_READS]; extra[1] = (int64_t)x->ctr[F2Q_UMI_FAILED];
    return x->ctr[F2Q_UMI_OVERFLOW] ? -1 : (long long)x->rehashes;
}
// pairs the set holds (the counter) and slots that are occupied (counted)
void uemu_set_info(void *h, uint64_t *held, uint64_t *occupied, uint64_t *slots)
{
    UEmu *x = (UEmu *)h;
    *held = x->ctr[F2Q_UMI_HELD]; *slots = x->slots.size(); *occupied = 0;
    for (unsigned long long k : x->slots) if (k != KEY_EMPTY) ++*occupied;
}

void uemu_reset(void *h)
{
    UEmu *x = (UEmu *)h;
    emu_reset(x->e);
    std::fill(x->slots.begin(), x->slots.end(), KEY_EMPTY);
    std::fill(x->reads.begin(), x->reads.end(), 0u);
    std::fill(x->umis.begin(), x->umis.end(), 0ull);
    std::fill(x->ctr.begin(), x->ctr.end(), 0ull);
}

}

#ifdef F2Q_UMI_EMU_MAIN
// 40 guides, 3 000 reads in blocks of 100 from a set of 64 slots: the set's own books must agree
int main()
{
    uint64_t z = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { z ^= z << 13; z ^= z >> 7; z ^= z << 17; return z; };
    const int NG = 40, GL = 20, RL = 36, S = 20, UL = 8;
    std::string seqs; std::vector<uint32_t> offs(1, 0);
    for (int g = 0; g < NG; g++) { for (int j = 0; j < GL; j++) seqs += "ACGT"[rnd() & 3]; offs.push_back((uint32_t)seqs.size()); }
    f2q_params p; memset(&p, 0, sizeof p);
    p.mode = 0; p.miss = 1; p.phred = 30; p.length = GL; p.n_start = 1; p.start[0] = 0; p.qual_up = p.qual_down = 30;
    void *h = uemu_create(&p, S, UL, 64);
    if (!h) return 2;
    uemu_set_features(h, seqs.data(), offs.data(), NG);
    for (int b = 0; b < 30; b++) {
        std::string fq;
        for (int i = 0; i < 100; i++) {
            std::string s = seqs.substr((size_t)(rnd() % NG) * GL, GL), q(RL, 'I');
            if (rnd() % 8 == 0) s[rnd() % GL] = 'N';
            for (int j = GL; j < RL; j++) s += "ACGT"[rnd() & 3];
            if (rnd() % 10 == 0) s[S + rnd() % UL] = 'N';
            if (rnd() % 10 == 0) q[S + rnd() % UL] = '#';
            if (rnd() % 10 == 0) { s.resize(S + rnd() % UL); q.resize(s.size()); }
            fq += "@r\n" + s + "\n+\n" + q + "\n";
        }
        if (uemu_count_block(h, (const uint8_t *)fq.data(), fq.size()) != fq.size()) return 3;
    }
    std::vector<int64_t> counts(NG), umis(NG); int64_t stats[5], extra[2];
    const long long rehashes = uemu_read(h, counts.data(), stats, umis.data(), extra);
    uint64_t held, occupied, slots; uemu_set_info(h, &held, &occupied, &slots);
    int64_t sum = 0; for (int64_t v : umis) sum += v;
    printf("reads %lld assigned %lld umi_reads %lld umi_failed %lld pairs %lld slots %llu rehashes %lld\n", (long long)stats[0],
           (long long)(stats[1] + stats[2]), (long long)extra[0], (long long)extra[1], (long long)sum, (unsigned long long)slots, rehashes);
    const bool ok = rehashes >= 3 && stats[0] == 3000 && extra[0] + extra[1] == stats[1] + stats[2] && extra[0] > 0 && extra[1] > 0 &&
                    (uint64_t)sum == held && held == occupied && 2 * held <= slots;
    uemu_destroy(h);
    return ok ? 0 : 1;
}
#endif
