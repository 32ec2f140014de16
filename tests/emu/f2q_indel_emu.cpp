// tests/emu/f2q_indel_emu.cpp -- TEST INFRASTRUCTURE.  The per-lane logic of k_count_indel (indel_read with its staged and
// unstaged span builders and indel_decide, 2fast2q_amd/csrc/f2q_device.h) and the host builder of the deletion-variant
// table (indel_build, f2q_host.h) compiled with g++ and run record by record over the existing emulation (f2q_emu.cpp,
// included whole), so the CPU suite can check them against the plain-Python rule of tests/indel_cases.py.  The product
// never uses this file.
// A record is staged as the kernel stages it -- when (offset & 3) + length <= 192 for both lines, the offsets being those
// of the text, as the device packer hands them on -- into two heap buffers of exactly the words the line covers, so that
// a sanitizer sees a span builder that steps outside them.
// -DF2Q_INDEL_EMU_MAIN: a stand-alone program (for -fsanitize=address,undefined builds): the removed-base keys for every L
// and p against a byte-by-byte builder, and the span of [s, s + L + 1) at every alignment and every line length up to the
// staging limit, staged against unstaged.
#include "f2q_emu.cpp"

#define IEMU_LINE_BYTES 192u             // 4 * F2Q_GEN_WORDS (f2q_count_kernels.h)

struct IEmu {
    Emu *e = nullptr;
    IndelDev d{};
    IndelTable tab;
    std::vector<unsigned long long> ctr;     // del_counts[nf], ins_counts[nf], del_pos[L], ins_pos[L], totals[4]
    uint64_t staged = 0, walked = 0;
};

static void iemu_bind(IEmu *x, const HostIndex &ix)
{
    const uint64_t nf = std::max<uint64_t>(ix.n_features, 1), L = (uint64_t)x->e->run.length;
    indel_build(ix, (int)L, x->tab);
    x->ctr.assign(2 * nf + 2 * L + F2Q_INDEL_TOTALS, 0ull);
    x->d.var_keys = x->tab.keys.data(); x->d.var_vals = x->tab.vals.data(); x->d.var_bits = x->tab.bits;
    x->d.del_counts = x->ctr.data(); x->d.ins_counts = x->ctr.data() + nf;
    x->d.del_pos = x->ctr.data() + 2 * nf; x->d.ins_pos = x->d.del_pos + L; x->d.totals = x->d.ins_pos + L;
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

void *iemu_create(const f2q_params *p)
{
    if (p->mode != 0 || p->n_start != 1 || p->length < 2 || p->length > F2Q_REG_MAXLEN) return nullptr;
    Emu *e = (Emu *)emu_create(p);
    if (!e) return nullptr;
    IEmu *x = new IEmu();
    x->e = e;
    iemu_bind(x, HostIndex());                                   // (no library yet: an empty table)
    return x;
}
void iemu_destroy(void *h) { IEmu *x = (IEmu *)h; emu_destroy(x->e); delete x; }

void iemu_set_features(void *h, const char *seqs, const uint32_t *offs, uint32_t n)
{
    IEmu *x = (IEmu *)h;
    emu_set_features(x->e, seqs, offs, n);
    iemu_bind(x, x->e->ix);
}

// what a lane of k_count_indel does, record by record.  layout 0: as the kernel decides (a record that fits is staged);
// 2: no record is staged (the byte-by-byte span on the text where it lies).
// per_read != nullptr: 4 bytes per record -- verdict + 1 (0: not tried), position, the feature's low 16 bits
size_t iemu_count_block(void *h, const uint8_t *buf, size_t n, int layout, uint8_t *per_read)
{
    IEmu *x = (IEmu *)h;
    Emu *e = x->e;
    std::vector<Rec> recs;
    const size_t used = frame_fastq(buf, n, recs);
    Accum acc{e->acc.data(), e->acc.data() + e->ix.n_features, nullptr, nullptr, nullptr, nullptr};
    for (size_t i = 0; i < recs.size(); i++) {
        const Rec &r = recs[i];
        const uint32_t ms = (uint32_t)(r.seq - buf) & 3u, mq = (uint32_t)(r.qual - buf) & 3u;
        const bool staged = layout != 2 && ms + r.len <= IEMU_LINE_BYTES && mq + r.qlen <= IEMU_LINE_BYTES;
        uint32_t *sw = staged ? stage_exact(r.seq, ms, r.len) : nullptr, *qw = staged ? stage_exact(r.qual, mq, r.qlen) : nullptr;
        uint32_t id = 0; int pos = 0;
        const int v = indel_read<const uint8_t *>(e->run, e->lib, e->ec, acc, x->d, sw, qw, ms, mq, r.seq, r.qual, (int)r.len, (int)r.qlen,
                                                  e->reads_seen + i, acc.stats, id, pos);
        free(sw); free(qw);
        const bool hit = v == F2Q_INDEL_DEL || v == F2Q_INDEL_INS;
        if (v != F2Q_INDEL_NOT_TRIED) x->d.totals[0]++;
        if (v == F2Q_INDEL_DEL) { x->d.del_counts[id]++; x->d.del_pos[pos]++; x->d.totals[1]++; }
        if (v == F2Q_INDEL_INS) { x->d.ins_counts[id]++; x->d.ins_pos[pos]++; x->d.totals[2]++; }
        if (v == F2Q_INDEL_AMBIGUOUS) x->d.totals[3]++;
        if (per_read) { per_read[4 * i] = (uint8_t)(v + 1); per_read[4 * i + 1] = (uint8_t)(hit ? pos : 0); per_read[4 * i + 2] = (uint8_t)(hit ? id : 0); per_read[4 * i + 3] = (uint8_t)(hit ? id >> 8 : 0); }
        (staged ? x->staged : x->walked)++;
    }
    e->reads_seen += recs.size(); e->general += recs.size();
    return used;
}

// counts[nf], stats[5], del_counts[nf], ins_counts[nf], del_pos[L], ins_pos[L], totals[4]; layout[2]: records staged / read where they lie
void iemu_read(void *h, int64_t *counts, int64_t *stats, int64_t *dels, int64_t *inss, int64_t *del_pos, int64_t *ins_pos, int64_t *totals, uint64_t *layout)
{
    IEmu *x = (IEmu *)h;
    emu_read_counts(x->e, counts, stats, nullptr, nullptr);
    const uint64_t nf = x->e->ix.n_features; const int L = x->e->run.length;
    for (uint64_t f = 0; f < nf; f++) { dels[f] = (int64_t)x->d.del_counts[f]; inss[f] = (int64_t)x->d.ins_counts[f]; }
    for (int p = 0; p < L; p++) { del_pos[p] = (int64_t)x->d.del_pos[p]; ins_pos[p] = (int64_t)x->d.ins_pos[p]; }
    for (int k = 0; k < F2Q_INDEL_TOTALS; k++) totals[k] = (int64_t)x->d.totals[k];
    layout[0] = x->staged; layout[1] = x->walked;
}

// the deletion-variant table as the host built it: its slots, and entry i of the occupied ones (key, value)
uint64_t iemu_table_slots(void *h) { return ((IEmu *)h)->tab.keys.size(); }
void iemu_table_info(void *h, uint64_t out[3]) { IEmu *x = (IEmu *)h; out[0] = x->tab.candidates; out[1] = x->tab.variants; out[2] = x->tab.shared; }
void iemu_table_dump(void *h, uint64_t *keys, uint64_t *vals)
{
    IEmu *x = (IEmu *)h;
    for (size_t i = 0; i < x->tab.keys.size(); i++) { keys[i] = x->tab.keys[i]; vals[i] = x->tab.vals[i]; }
}

}

#ifdef F2Q_INDEL_EMU_MAIN
int main()
{
    long long keys = 0, spans = 0, bad = 0;
    uint64_t x = 0x9E3779B97F4A7C15ull;
    // the key of the L bases that stay when base p leaves L + 1, against its bases one by one
    for (int L = 2; L <= 31; L++) for (int rep = 0; rep < 40; rep++) {
        uint8_t c[32]; uint64_t w = 0;
        for (int j = 0; j <= L; j++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; c[j] = (uint8_t)(rep == 0 ? 3 : rep == 1 ? 0 : x & 3); w |= (uint64_t)c[j] << (2 * j); }
        for (int p = 0; p < L; p++) {
            uint64_t want = 0; int at = 0;
            for (int j = 0; j <= L; j++) if (j != p) { want |= (uint64_t)c[j] << (2 * at); at++; }
            bad += indel_removed(w, p, L) != want;
            keys++;
        }
        for (int p = 0; p < L; p++) {                                // a feature of L bases losing base p: L - 1 stay
            uint64_t want = 0; int at = 0; const uint64_t k = w & indel_low2(L);
            for (int j = 0; j < L; j++) if (j != p) { want |= (uint64_t)c[j] << (2 * at); at++; }
            bad += indel_removed(k, p, L - 1) != want;
            keys++;
        }
    }
    // the three words of [s, s + lim): built from the staged words against built byte by byte, from buffers of exactly the staged size
    const char alphabet[] = "ACGTACGTACGTacgtNn.-*!#5=>I~";
    for (uint32_t n = 0; n <= IEMU_LINE_BYTES; n++) {
        for (uint32_t ms = 0; ms < 4; ms++) for (uint32_t mq = 0; mq < 4; mq++) {
            if (ms + n > IEMU_LINE_BYTES || mq + n > IEMU_LINE_BYTES) continue;
            std::vector<uint8_t> seq(n + 1), qual(n + 1);
            for (uint32_t i = 0; i < n; i++) {
                x ^= x << 13; x ^= x >> 7; x ^= x << 17;
                seq[i] = (uint8_t)alphabet[x % (sizeof alphabet - 1)];
                qual[i] = (x >> 20) % 9 == 0 ? (uint8_t)(33 + (x >> 24) % 30) : (uint8_t)'I';
                if ((x >> 40) % 61 == 0) { seq[i] = (uint8_t)(x >> 48); qual[i] = (uint8_t)(x >> 56); }
            }
            uint32_t *sw = stage_exact(seq.data(), ms, n), *qw = stage_exact(qual.data(), mq, n);
            uint8_t *se = (uint8_t *)malloc(n ? n : 1), *qe = (uint8_t *)malloc(n ? n : 1);      // the lines alone: a byte past them is out of bounds
            memcpy(se, seq.data(), n); memcpy(qe, qual.data(), n);
            for (int s = 0; s <= (int)n; s += (n > 70 && s > 3 && s + 70 < (int)n) ? 17 : 1) {
                const int room = (int)n - s;
                const int lims[4] = {room < 32 ? room : 32, room < 21 ? room : 21, room < 3 ? room : 3, 0};
                for (int k = 0; k < 4; k++) for (int thr = 32; thr <= 72; thr += 40) {
                    StaggerSpan sp;
                    stagger_span(sw, qw, ms, mq, s, lims[k], thr, sp);
                    uint64_t w, nm, qm;
                    indel_span_bytes<const uint8_t *>(se, qe, s, lims[k], thr, w, nm, qm);
                    bad += sp.lo != w || sp.hi != 0 || sp.nmask != nm || sp.qmask != qm;
                    spans++;
                }
            }
            free(sw); free(qw); free(se); free(qe);
        }
    }
    printf("indel: %lld removed-base keys, %lld spans built from buffers of their staged size, %lld mismatches\n", keys, spans, bad);
    return bad == 0 && spans > 0 && keys > 0 ? 0 : 1;
}
#endif
