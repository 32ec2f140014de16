// tests/emu/f2q_strand_emu.cpp -- TEST INFRASTRUCTURE.  The per-lane logic of k_count_strand (strand_read with mirror_line,
// StrandBytes and StrandHook around general_read, 2fast2q_amd/csrc/f2q_device.h) compiled with g++ and run record by record
// over the existing emulation (f2q_emu.cpp, included whole), so the CPU suite can check it against the plain-Python rule of
// tests/strand_cases.py.  The product never uses this file.
// A record is staged as the kernel stages it -- when (offset & 3) + length <= 192 for both lines, the offsets being those
// of the text, as the device packer hands them on -- into two heap buffers of exactly the words the line covers, so that
// a sanitizer sees a mirror that steps outside them.
// -DF2Q_STRAND_EMU_MAIN: a stand-alone program (for -fsanitize=address,undefined builds): mirror_line on every stageable
// line of the FASTQ files named on the command line, against a byte-by-byte mirror.
#include "f2q_emu.cpp"

#define SEMU_LINE_BYTES 192u             // 4 * F2Q_GEN_WORDS (f2q_count_kernels.h)

struct SEmu {
    Emu *e = nullptr;
    StrandDev d{};
    std::vector<unsigned long long> ctr;     // rev_counts[max(n_features, 1)] then extra[4]
    uint64_t staged = 0, walked = 0;
};

static void semu_bind(SEmu *x)
{
    const uint64_t nf = std::max<uint64_t>(x->e->ix.n_features, 1);
    x->ctr.assign(nf + 4, 0ull);
    x->d.rev_counts = x->ctr.data(); x->d.extra = x->ctr.data() + nf;
}

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

void *semu_create(const f2q_params *p, int32_t mode)
{
    if (p->mode != 0 || (mode != 1 && mode != 2)) return nullptr;
    Emu *e = (Emu *)emu_create(p);
    if (!e) return nullptr;
    SEmu *x = new SEmu();
    x->e = e; x->d.mode = mode;
    semu_bind(x);
    return x;
}
void semu_destroy(void *h) { SEmu *x = (SEmu *)h; emu_destroy(x->e); delete x; }

void semu_set_features(void *h, const char *seqs, const uint32_t *offs, uint32_t n)
{
    SEmu *x = (SEmu *)h;
    emu_set_features(x->e, seqs, offs, n);
    semu_bind(x);
}

// what a lane of k_count_strand does, record by record.  walk_all != 0: no record is staged (the accessor everywhere)
size_t semu_count_block(void *h, const uint8_t *buf, size_t n, int walk_all)
{
    SEmu *x = (SEmu *)h;
    Emu *e = x->e;
    std::vector<Rec> recs;
    const size_t used = frame_fastq(buf, n, recs);
    Accum acc{e->acc.data(), e->acc.data() + e->ix.n_features, nullptr, nullptr, nullptr, nullptr};
    for (size_t i = 0; i < recs.size(); i++) {
        const Rec &r = recs[i];
        const uint32_t ms = (uint32_t)(r.seq - buf) & 3u, mq = (uint32_t)(r.qual - buf) & 3u;
        const bool staged = !walk_all && ms + r.len <= SEMU_LINE_BYTES && mq + r.qlen <= SEMU_LINE_BYTES;
        uint32_t *sw = staged ? stage_exact(r.seq, ms, r.len) : nullptr, *qw = staged ? stage_exact(r.qual, mq, r.qlen) : nullptr;
        if (x->d.mode == 2) strand_read<true, const uint8_t *>(e->run, e->lib, e->ec, acc, x->d, sw, qw, ms, mq, r.seq, r.qual, (int)r.len, (int)r.qlen, e->reads_seen + i, acc.stats, x->d.extra);
        else strand_read<false, const uint8_t *>(e->run, e->lib, e->ec, acc, x->d, sw, qw, ms, mq, r.seq, r.qual, (int)r.len, (int)r.qlen, e->reads_seen + i, acc.stats, x->d.extra);
        free(sw); free(qw);
        (staged ? x->staged : x->walked)++;
    }
    e->reads_seen += recs.size(); e->general += recs.size();
    return used;
}

// counts[nf], stats[5], rev_counts[nf], extra[4]; layout[2]: records staged / walked where they lie
void semu_read(void *h, int64_t *counts, int64_t *stats, int64_t *rev, int64_t *extra, uint64_t *layout)
{
    SEmu *x = (SEmu *)h;
    emu_read_counts(x->e, counts, stats, nullptr, nullptr);
    const uint64_t nf = x->e->ix.n_features;
    for (uint64_t f = 0; f < nf; f++) rev[f] = (int64_t)x->ctr[f];
    for (int k = 0; k < 4; k++) extra[k] = (int64_t)x->d.extra[k];
    layout[0] = x->staged; layout[1] = x->walked;
}

// mirror_line on one line staged at misalignment mis: the mirrored bytes in out (at least n), their number returned
int32_t semu_mirror(const uint8_t *line, uint32_t mis, int32_t n, int32_t comp, uint8_t *out)
{
    uint32_t *w = stage_exact(line, mis, (uint32_t)n);
    if (comp) mirror_line<true>(w, mis, n); else mirror_line<false>(w, mis, n);
    memcpy(out, reinterpret_cast<const uint8_t *>(w) + mis, (size_t)n);
    free(w);
    return n;
}

}

#ifdef F2Q_STRAND_EMU_MAIN
// byte by byte, as include/f2q.h states it: reversed, complemented by comp8, rstrip()-ed again
static std::string plain_mirror(const uint8_t *p, uint32_t n, bool comp)
{
    std::string out;
    for (uint32_t j = 0; j < n; j++) { const uint8_t c = p[n - 1 - j]; out += (char)(comp ? comp8(c) : c); }
    out.resize(rstrip_len((const uint8_t *)out.data(), out.size()));
    return out;
}
int main(int argc, char **argv)
{
    long long lines = 0, skipped = 0, bad = 0, blanks = 0;
    for (int a = 1; a < argc; a++) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        std::vector<uint8_t> text;
        uint8_t chunk[65536];
        for (size_t got; (got = fread(chunk, 1, sizeof chunk, f)) > 0;) text.insert(text.end(), chunk, chunk + got);
        fclose(f);
        std::vector<Rec> recs;
        frame_fastq(text.data(), text.size(), recs);
        for (const Rec &r : recs) {
            const uint8_t *line[2] = {r.seq, r.qual}; const uint32_t len[2] = {r.len, r.qlen};
            for (int k = 0; k < 2; k++) {
                const uint32_t mis = (uint32_t)(line[k] - text.data()) & 3u;
                if (mis + len[k] > SEMU_LINE_BYTES) { skipped++; continue; }
                std::vector<uint8_t> out(len[k] + 1);
                const int32_t n = semu_mirror(line[k], mis, (int32_t)len[k], k == 0, out.data());
                const std::string want = plain_mirror(line[k], len[k], k == 0);
                bad += n != (int32_t)want.size() || memcmp(out.data(), want.data(), want.size()) != 0;
                blanks += want.size() != len[k];
                lines++;
            }
        }
    }
    printf("mirror_line: %lld lines mirrored in buffers of their staged size (%lld with leading blanks), %lld too long to stage, %lld mismatches\n",
           lines, blanks, skipped, bad);
    return bad == 0 && lines > 0 ? 0 : 1;
}
#endif
