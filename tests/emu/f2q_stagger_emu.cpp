// tests/emu/f2q_stagger_emu.cpp -- TEST INFRASTRUCTURE.  The per-lane logic of k_count_stagger (stagger_read with its walk
// and span layouts, 2fast2q_amd/csrc/f2q_device.h) compiled with g++ and run record by record over the existing emulation
// (f2q_emu.cpp, included whole), so the CPU suite can check it against the plain-Python rule of tests/stagger_cases.py.
// The product never uses this file.
// A record is staged as the kernel stages it -- when (offset & 3) + length <= 192 for both lines, the offsets being those
// of the text, as the device packer hands them on -- into two heap buffers of exactly the words the line covers, so that
// a sanitizer sees a span builder that steps outside them.
// -DF2Q_STAGGER_EMU_MAIN: a stand-alone program (for -fsanitize=address,undefined builds): stagger_span on every alignment
// and every line length up to the staging limit, against a byte-by-byte builder.
#include "f2q_emu.cpp"

#define GEMU_LINE_BYTES 192u             // 4 * F2Q_GEN_WORDS (f2q_count_kernels.h)

struct GEmu {
    Emu *e = nullptr;
    StaggerDev d{};
    std::vector<unsigned long long> hist;    // [2][n + 1]
    uint64_t staged = 0, walked = 0;
};

// the words a line of n bytes at misalignment mis is staged in, exactly: stage_line's layout (byte i at offset mis + i)
static uint32_t *stage_exact(const uint8_t *line, uint32_t mis, uint32_t n)
{
    const uint32_t nw = (mis + n + 3u) >> 2;
    uint32_t *w = (uint32_t *)malloc(nw ? (size_t)nw * 4 : 1);
    if (nw) memset(w, 0xA5, (size_t)nw * 4);
    memcpy(reinterpret_cast<uint8_t *>(w) + mis, line, n);
    return w;
}

extern "C" {

void *gemu_create(const f2q_params *p, int32_t n)
{
    if (p->mode != 0 || n < 1 || n > F2Q_STAGGER_MAX || p->n_start != 1) return nullptr;
    Emu *e = (Emu *)emu_create(p);
    if (!e) return nullptr;
    GEmu *x = new GEmu();
    x->e = e; x->d.n = n;
    x->hist.assign(2 * ((size_t)n + 1), 0ull);
    x->d.hist = x->hist.data();
    return x;
}
void gemu_destroy(void *h) { GEmu *x = (GEmu *)h; emu_destroy(x->e); delete x; }

void gemu_set_features(void *h, const char *seqs, const uint32_t *offs, uint32_t n)
{
    GEmu *x = (GEmu *)h;
    emu_set_features(x->e, seqs, offs, n);
}

// what a lane of k_count_stagger does, record by record.  layout 0: as the kernel decides (span where it applies);
// 1: F2Q_STAGGER_WALK=1 (staged records walked); 2: no record is staged (the walk on the text where it lies).
// per_read != nullptr: 4 bytes per record -- verdict, offset + 1 (0: none), the feature's low 16 bits
size_t gemu_count_block(void *h, const uint8_t *buf, size_t n, int layout, uint8_t *per_read)
{
    GEmu *x = (GEmu *)h;
    Emu *e = x->e;
    std::vector<Rec> recs;
    const size_t used = frame_fastq(buf, n, recs);
    unsigned long long *counts = e->acc.data(), *st = e->acc.data() + e->ix.n_features;
    x->d.walk = layout == 1;
    for (size_t i = 0; i < recs.size(); i++) {
        const Rec &r = recs[i];
        const uint32_t ms = (uint32_t)(r.seq - buf) & 3u, mq = (uint32_t)(r.qual - buf) & 3u;
        const bool staged = layout != 2 && ms + r.len <= GEMU_LINE_BYTES && mq + r.qlen <= GEMU_LINE_BYTES;
        uint32_t *sw = staged ? stage_exact(r.seq, ms, r.len) : nullptr, *qw = staged ? stage_exact(r.qual, mq, r.qlen) : nullptr;
        uint32_t id = 0; int off = -1;
        const int v = stagger_read<const uint8_t *>(e->run, e->lib, x->d, sw, qw, ms, mq, r.seq, r.qual, (int)r.len, (int)r.qlen, id, off);
        free(sw); free(qw);
        st[0]++; st[v]++;
        if (v <= 2) { counts[id]++; x->hist[(size_t)(v - 1) * (x->d.n + 1) + off]++; }
        if (per_read) { per_read[4 * i] = (uint8_t)v; per_read[4 * i + 1] = (uint8_t)(off + 1); per_read[4 * i + 2] = (uint8_t)(v <= 2 ? id : 0); per_read[4 * i + 3] = (uint8_t)(v <= 2 ? id >> 8 : 0); }
        (staged ? x->staged : x->walked)++;
    }
    e->reads_seen += recs.size(); e->general += recs.size();
    return used;
}

// counts[nf], stats[5], perfect[n + 1], imperfect[n + 1]; layout[2]: records staged / walked where they lie
void gemu_read(void *h, int64_t *counts, int64_t *stats, int64_t *perfect, int64_t *imperfect, uint64_t *layout)
{
    GEmu *x = (GEmu *)h;
    emu_read_counts(x->e, counts, stats, nullptr, nullptr);
    for (int d = 0; d <= x->d.n; d++) { perfect[d] = (int64_t)x->hist[d]; imperfect[d] = (int64_t)x->hist[x->d.n + 1 + d]; }
    layout[0] = x->staged; layout[1] = x->walked;
}

}

#ifdef F2Q_STAGGER_EMU_MAIN
// byte by byte: what stagger_span must give for positions [s, s + lim) of the two lines
static StaggerSpan plain_span(const uint8_t *seq, const uint8_t *qual, int s, int lim, int thr)
{
    StaggerSpan sp{0, 0, 0, 0};
    for (int p = 0; p < lim; p++) {
        uint32_t c = base_code(up8(seq[s + p]));
        if (c > 3u) { sp.nmask |= 1ull << p; c = 0; }
        if (p < 32) sp.lo |= (uint64_t)c << (2 * p); else sp.hi |= (uint64_t)c << (2 * (p - 32));
        if (thr >= 33 && q_fails(qual[s + p], thr)) sp.qmask |= 1ull << p;
    }
    return sp;
}
int main()
{
    long long spans = 0, bad = 0, keys = 0;
    uint64_t x = 0x9E3779B97F4A7C15ull;
    const char alphabet[] = "ACGTACGTACGTacgtNn.-*!#5=>I~";
    for (uint32_t n = 0; n <= GEMU_LINE_BYTES; n++) {
        for (uint32_t ms = 0; ms < 4; ms++) for (uint32_t mq = 0; mq < 4; mq++) {
            if (ms + n > GEMU_LINE_BYTES || mq + n > GEMU_LINE_BYTES) continue;
            std::vector<uint8_t> seq(n + 1), qual(n + 1);
            for (uint32_t i = 0; i < n; i++) {
                x ^= x << 13; x ^= x >> 7; x ^= x << 17;
                seq[i] = (uint8_t)alphabet[x % (sizeof alphabet - 1)];
                qual[i] = (x >> 20) % 9 == 0 ? (uint8_t)(33 + (x >> 24) % 30) : (uint8_t)'I';
                if ((x >> 40) % 61 == 0) { seq[i] = (uint8_t)(x >> 48); qual[i] = (uint8_t)(x >> 56); }
            }
            uint32_t *sw = stage_exact(seq.data(), ms, n), *qw = stage_exact(qual.data(), mq, n);
            // every start the line leaves room for (the far end included), the longest span there and a short one
            for (int s = 0; s <= (int)n; s += (n > 70 && s > 3 && s + 70 < (int)n) ? 17 : 1) {
                const int room = (int)n - s;
                const int lims[3] = {room < 63 ? room : 63, room < 21 ? room : 21, room < 1 ? room : 1};
                for (int k = 0; k < 3; k++) for (int thr = 32; thr <= 72; thr += 40) {
                    StaggerSpan got;
                    stagger_span(sw, qw, ms, mq, s, lims[k], thr, got);
                    const StaggerSpan want = plain_span(seq.data(), qual.data(), s, lims[k], thr);
                    bad += got.lo != want.lo || got.hi != want.hi || got.nmask != want.nmask || got.qmask != want.qmask;
                    spans++;
                    // the key of every window inside the span, against its bases one by one
                    for (int L = 1; L <= 31 && k == 0 && thr == 32; L += 6) for (int d = 0; d <= 32 && d + L <= lims[k]; d++) {
                        uint64_t key = 0;
                        for (int j = 0; j < L; j++) { uint32_t c = base_code(up8(seq[s + d + j])); key |= (uint64_t)(c > 3u ? 0u : c) << (2 * j); }
                        bad += stagger_key(got, d, L) != key;
                        keys++;
                    }
                }
            }
            free(sw); free(qw);
        }
    }
    for (uint64_t m = 1; m < (1ull << 31); m = m * 3 + 1) {
        uint64_t want = 0;
        for (int j = 0; j < 31; j++) if ((m >> j) & 1) want |= 1ull << (2 * j);
        bad += stagger_spread(m & 0x7FFFFFFFull) != want;
    }
    printf("stagger_span: %lld spans built from buffers of their staged size, %lld window keys, %lld mismatches\n", spans, keys, bad);
    return bad == 0 && spans > 0 ? 0 : 1;
}
#endif
