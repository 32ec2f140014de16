// tests/emu/f2q_demux_emu.cpp -- TEST INFRASTRUCTURE.  The per-lane logic of k_count_demux (demux_decide / demux_find and
// general_read with a DemuxHook, 2fast2q_amd/csrc/f2q_device.h) and the host's table builder (demux_validate / demux_build,
// f2q_host.h) compiled with g++ and run record by record over the existing emulation (f2q_emu.cpp, included whole), so the
// CPU suite can check them against the plain-Python rule of tests/demux_cases.py.  The product never uses this file.
// -DF2Q_DEMUX_EMU_MAIN: a stand-alone program over a built-in sample (for -fsanitize=address,undefined builds).
#include "f2q_emu.cpp"

struct DEmu {
    Emu *e = nullptr;                        // null: a table alone (demu_table)
    DemuxTable tab;
    DemuxDev d{};
    std::vector<unsigned long long> matrix, ctr;     // ctr: sstats[(n + 1) * 5] then verdicts[5]
};

static void demu_bind(DEmu *x)
{
    const uint64_t nf = x->e ? std::max<uint64_t>(x->e->ix.n_features, 1) : 1, rows = (uint64_t)x->d.n + 1;
    x->matrix.assign(rows * nf, 0ull); x->ctr.assign(rows * 5 + 5, 0ull);
    x->d.table = x->tab.slots.data(); x->d.mask = x->tab.mask; x->d.n_features = x->e ? x->e->ix.n_features : 0;
    x->d.matrix = x->matrix.data(); x->d.sstats = x->ctr.data(); x->d.verdicts = x->ctr.data() + rows * 5;
}

static DEmu *demu_make(Emu *e, const char *seqs, uint32_t n, int32_t length, int32_t start, int32_t miss, std::string &err)
{
    std::string up;
    if (demux_validate(seqs, n, length, start, miss, up, err)) return nullptr;
    DEmu *x = new DEmu();
    x->e = e;
    demux_build(up, n, length, miss, x->tab);
    x->d.start = start; x->d.length = length; x->d.miss = miss; x->d.n = n;
    demu_bind(x);
    return x;
}

extern "C" {

// f2q_set_sample_barcodes' argument check: the F2Q_E* code, the message in msg
int demu_validate(const char *seqs, uint32_t n, int32_t length, int32_t start, int32_t miss, char *msg, size_t cap)
{
    std::string up, err;
    const int rc = demux_validate(seqs, n, length, start, miss, up, err);
    if (msg && cap) { strncpy(msg, err.c_str(), cap - 1); msg[cap - 1] = 0; }
    return rc;
}

// a table alone
void *demu_table(const char *seqs, uint32_t n, int32_t length, int32_t start, int32_t miss)
{
    std::string err;
    return demu_make(nullptr, seqs, n, length, start, miss, err);
}
void demu_info(void *h, uint64_t *slots, uint32_t *entries, uint32_t *ambiguous)
{
    DEmu *x = (DEmu *)h;
    *slots = x->tab.slots.size(); *entries = x->tab.entries; *ambiguous = x->tab.ambiguous;
}
void demu_slots(void *h, uint64_t *out)
{
    DEmu *x = (DEmu *)h;
    for (size_t i = 0; i < x->tab.slots.size(); i++) out[i] = x->tab.slots[i];
}
// the device rule on one record: the verdict, *sample
int demu_decide(void *h, int32_t phred, const uint8_t *seq, int32_t r, const uint8_t *qual, int32_t qn, uint32_t *sample)
{
    DEmu *x = (DEmu *)h;
    return demux_decide(x->d, x->d.table, phred_threshold(phred), seq, r, qual, qn, *sample);
}

// a counting context: what a lane of k_count_demux does, record by record
void *demu_create(const f2q_params *p, const char *seqs, uint32_t n, int32_t length, int32_t start, int32_t miss)
{
    if (p->mode != 0) return nullptr;
    Emu *e = (Emu *)emu_create(p);
    if (!e) return nullptr;
    std::string err;
    DEmu *x = demu_make(e, seqs, n, length, start, miss, err);
    if (!x) emu_destroy(e);
    return x;
}
void demu_destroy(void *h) { DEmu *x = (DEmu *)h; if (x->e) emu_destroy(x->e); delete x; }

void demu_set_features(void *h, const char *seqs, const uint32_t *offs, uint32_t n)
{
    DEmu *x = (DEmu *)h;
    emu_set_features(x->e, seqs, offs, n);
    demu_bind(x);
}

size_t demu_count_block(void *h, const uint8_t *buf, size_t n)
{
    DEmu *x = (DEmu *)h;
    Emu *e = x->e;
    std::vector<Rec> recs;
    const size_t used = frame_fastq(buf, n, recs);
    Accum acc{e->acc.data(), e->acc.data() + e->ix.n_features, nullptr, nullptr, nullptr, nullptr};
    for (size_t i = 0; i < recs.size(); i++) {
        const Rec &r = recs[i];
        uint32_t sample = x->d.n;
        const int v = demux_decide(x->d, x->d.table, e->run.thr, r.seq, (int)r.len, r.qual, (int)r.qlen, sample);
        x->d.verdicts[v]++;
        const DemuxHook hook{x->d.matrix + (unsigned long long)sample * x->d.n_features};
        unsigned long long one[5] = {0, 0, 0, 0, 0};
        general_read<const uint8_t *, true, false>(e->run, e->lib, e->ec, acc, r.seq, (int)r.len, r.qual, (int)r.qlen, e->reads_seen + i, one, nullptr, 0, 0, hook);
        for (int k = 0; k < 5; k++) { acc.stats[k] += one[k]; x->d.sstats[sample * 5u + (uint32_t)k] += one[k]; }
    }
    e->reads_seen += recs.size(); e->general += recs.size();
    return used;
}

// counts[nf], stats[5], matrix[(n + 1) * nf], sstats[(n + 1) * 5], verdicts[5]
void demu_read(void *h, int64_t *counts, int64_t *stats, int64_t *matrix, int64_t *sstats, int64_t *verdicts)
{
    DEmu *x = (DEmu *)h;
    emu_read_counts(x->e, counts, stats, nullptr, nullptr);
    const uint64_t nf = x->e->ix.n_features, rows = (uint64_t)x->d.n + 1;
    for (uint64_t i = 0; i < rows * nf; i++) matrix[i] = (int64_t)x->matrix[i];
    for (uint64_t i = 0; i < rows * 5; i++) sstats[i] = (int64_t)x->ctr[i];
    for (int k = 0; k < 5; k++) verdicts[k] = (int64_t)x->ctr[rows * 5 + k];
}

void demu_reset(void *h)
{
    DEmu *x = (DEmu *)h;
    emu_reset(x->e);
    std::fill(x->matrix.begin(), x->matrix.end(), 0ull);
    std::fill(x->ctr.begin(), x->ctr.end(), 0ull);
}

}

#ifdef F2Q_DEMUX_EMU_MAIN
// brute force on the bytes, as include/f2q.h states the rule
static int brute(const std::string &bcs, uint32_t n, int L, int M, const std::string &w, uint32_t &sample)
{
    uint32_t ones = 0, who = n;
    for (uint32_t b = 0; b < n; b++) {
        int d = 0;
        for (int j = 0; j < L; j++) d += up8((uint8_t)w[j]) != (uint8_t)bcs[(size_t)b * L + j];
        if (d == 0) { sample = b; return F2Q_DEMUX_EXACT; }
        if (d == 1) { ones++; who = b; }
    }
    sample = n;
    if (M == 1 && ones == 1) { sample = who; return F2Q_DEMUX_ONE; }
    if (M == 1 && ones > 1) return F2Q_DEMUX_AMBIGUOUS;
    return F2Q_DEMUX_NOMATCH;
}
// 40 barcodes of 6 bases (dense enough for every verdict), 20 000 windows over ACGTNacgt with cut and low-quality records
int main()
{
    uint64_t z = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { z ^= z << 13; z ^= z >> 7; z ^= z << 17; return z; };
    const int L = 6, S = 5; const uint32_t NB = 40;
    std::string bcs;
    for (uint32_t b = 0; b < NB; b++) for (;;) {
        std::string c; for (int j = 0; j < L; j++) c += "ACGT"[rnd() & 3];
        bool dup = false; for (uint32_t o = 0; o < b; o++) dup |= bcs.compare((size_t)o * L, L, c) == 0;
        if (!dup) { bcs += c; break; }
    }
    long long bad = 0, seen[5] = {0, 0, 0, 0, 0};
    for (int M = 0; M < 2; M++) {
        void *h = demu_table(bcs.data(), NB, L, S, M);
        if (!h) return 2;
        for (int i = 0; i < 20000; i++) {
            std::string s(S + L + 3, 'A'), q(S + L + 3, 'I');
            for (int j = 0; j < L; j++) s[S + j] = "ACGTACGTACGTACGTNacgt"[rnd() % 21];
            if (rnd() % 16 == 0) s.resize(S + rnd() % L);
            if (rnd() % 16 == 0) q.resize(S + rnd() % L);
            if (rnd() % 16 == 0) q[rnd() % q.size()] = '#';
            uint32_t got_s = 0, want_s = NB;
            const int got = demu_decide(h, 30, (const uint8_t *)s.data(), (int)s.size(), (const uint8_t *)q.data(), (int)q.size(), &got_s);
            int want = F2Q_DEMUX_UNREADABLE;
            bool readable = (int)s.size() >= S + L && (int)q.size() >= S + L;
            for (int j = S; readable && j < S + L; j++) readable = q[j] != '#';
            if (readable) want = brute(bcs, NB, L, M, s.substr(S, L), want_s);
            bad += got != want || got_s != want_s;
            seen[got]++;
        }
        demu_destroy(h);
    }
    printf("verdicts %lld %lld %lld %lld %lld, %lld mismatches\n", seen[0], seen[1], seen[2], seen[3], seen[4], bad);
    return bad == 0 && seen[0] && seen[1] && seen[2] && seen[3] && seen[4] ? 0 : 1;
}
#endif
