// tests/emu/f2q_umi_header_emu.cpp -- TEST INFRASTRUCTURE.  The host side of a header-UMI context (f2q_set_umi_header)
// compiled with g++ over the UMI emulation (f2q_umi_emu.cpp, included whole): header_umi_codes of f2q_device.h on one line,
// the host packer's array (frame_fastq + header_umis of f2q_host.h: what k_header_umi writes on the device), and what a
// lane of k_count_umi<READS, true> does with it -- general_read with a UmiHeaderHook that takes the record's entry from
// that array.  The product never uses this file.
// -DF2Q_UMI_HEADER_EMU_MAIN: a stand-alone program over built-in lines (for -fsanitize=address,undefined builds).
#include "f2q_umi_emu.cpp"

// every record through the byte-exact routine, its UMI taken from entry[position of the record in the block]
template <bool READS>
static size_t hemu_count(UEmu *x, const uint8_t *buf, size_t n, uint32_t sep, uint32_t length)
{
    Emu *e = x->e;
    std::vector<Rec> recs;
    const size_t used = frame_fastq(buf, n, recs);
    std::vector<unsigned long long> entry;
    header_umis(recs, recs.size(), sep, length, entry);
    uemu_reserve(x, recs.size());
    Accum acc{e->acc.data(), e->acc.data() + e->ix.n_features, nullptr, nullptr, nullptr, nullptr};
    for (size_t i = 0; i < recs.size(); i++) {
        unsigned long long ust[3] = {0, 0, 0};
        const UmiHeaderHook<READS> hook{&x->u, entry[i], ust};
        general_read<const uint8_t *, true, false>(e->run, e->lib, e->ec, acc, recs[i].seq, (int)recs[i].len, recs[i].qual, (int)recs[i].qlen,
                                                   e->reads_seen + i, acc.stats, nullptr, 0, 0, hook);
        x->ctr[F2Q_UMI_READS] += ust[0]; x->ctr[F2Q_UMI_FAILED] += ust[1]; x->ctr[F2Q_UMI_HELD] += ust[2];
    }
    e->reads_seen += recs.size(); e->general += recs.size();
    return used;
}

extern "C" {

// header_umi_codes on one line of n bytes: 1 and *codes, or 0
int hemu_parse(const uint8_t *line, uint32_t n, uint32_t sep, uint32_t length, uint32_t *codes)
{
    uint32_t w = 0;
    const bool ok = header_umi_codes<const uint8_t *>(line, n, sep, length, w);
    if (ok) *codes = w;
    return ok ? 1 : 0;
}

// the host packer's array for a FASTQ text: entries of the complete records into out[cap]; returns how many there are
size_t hemu_array(const uint8_t *buf, size_t n, uint32_t sep, uint32_t length, unsigned long long *out, size_t cap)
{
    std::vector<Rec> recs;
    frame_fastq(buf, n, recs);
    std::vector<unsigned long long> entry;
    header_umis(recs, recs.size(), sep, length, entry);
    for (size_t i = 0; i < entry.size() && i < cap; i++) out[i] = entry[i];
    return entry.size();
}

// a UEmu made by uemu_create(p, 0, length, min_slots); keep != 0: reads per pair
size_t hemu_count_block(void *h, const uint8_t *buf, size_t n, uint32_t sep, uint32_t length, int keep)
{
    UEmu *x = (UEmu *)h;
    x->keep_reads = keep != 0;
    return keep ? hemu_count<true>(x, buf, n, sep, length) : hemu_count<false>(x, buf, n, sep, length);
}

// the pairs of the set with their reads (0 when not kept), unsorted; returns how many
size_t hemu_pairs(void *h, uint32_t *feature, uint32_t *codes, uint32_t *reads, size_t cap)
{
    UEmu *x = (UEmu *)h;
    size_t k = 0;
    for (size_t s = 0; s < x->slots.size(); s++) {
        if (x->slots[s] == KEY_EMPTY) continue;
        if (k < cap) { feature[k] = (uint32_t)(x->slots[s] >> 32); codes[k] = (uint32_t)x->slots[s]; reads[k] = x->reads.empty() ? 0u : x->reads[s]; }
        k++;
    }
    return k;
}

}

#ifdef F2Q_UMI_HEADER_EMU_MAIN
// lines that end at every state of the parse, each in a heap buffer of exactly its length
int main()
{
    struct Case { const char *line; uint32_t sep, length; int ok; uint32_t codes; };
    const Case cases[] = {
        {"@r1_ACGTACGT", '_', 8, 1, 0xE4E4u}, {"@r1_acgtACGT \t", '_', 8, 1, 0xE4E4u}, {"@r1_ACGT+ACGT 1:N:0:1", '_', 8, 1, 0xE4E4u},
        {"@r1_+ACGTACGT", '_', 8, 1, 0xE4E4u}, {"@r1_AC+GT+ACGT", '_', 8, 0, 0}, {"@r1_ACGTACG", '_', 8, 0, 0}, {"@r1_ACGTACGTA", '_', 8, 0, 0},
        {"@r1_", '_', 8, 0, 0}, {"@", '_', 8, 0, 0}, {"", '_', 8, 0, 0}, {"@r1 1:N:0:1_ACGTACGT", '_', 8, 0, 0}, {"@r1_ACGTNCGT", '_', 8, 0, 0},
        {"@M0:7:FC:1:1101:100:200:ACGTACGT 1:N:0:ATCACG", ':', 8, 1, 0xE4E4u}, {"@x_TTTTTTTTTTTTTTTT", '_', 16, 1, 0xFFFFFFFFu},
        {"@x_AAAAAAAAAAAAAAAA\r", '_', 16, 1, 0u}, {"@x_AAAAAAAAAAAAAAAAA", '_', 16, 0, 0}, {"@r_1_ACGTACGTAAAA_ACGTACGT", '_', 8, 1, 0xE4E4u},
        {"   ", '_', 8, 0, 0}, {"_T", '_', 1, 1, 3u}};
    int bad = 0;
    for (const Case &c : cases) {
        const size_t n = strlen(c.line);
        std::vector<uint8_t> heap(c.line, c.line + n);
        uint32_t codes = 0;
        const int ok = hemu_parse(heap.data(), (uint32_t)n, c.sep, c.length, &codes);
        if (ok != c.ok || (ok && codes != c.codes)) { printf("line '%s': got %d %08x, want %d %08x\n", c.line, ok, codes, c.ok, c.codes); bad++; }
    }
    const char fq[] = "@a_ACGTACGT\nACGT\n+\nIIII\n@b\nACGT\n+\nIIII\n@c_TTTTTTTT 1\nAC\n+\nII";
    unsigned long long out[4] = {0, 0, 0, 0};
    const size_t n = hemu_array((const uint8_t *)fq, sizeof fq - 1, '_', 8, out, 4);
    if (n != 3 || out[0] != (F2Q_UMI_HDR_VALID | 0xE4E4u) || out[1] != 0ull || out[2] != (F2Q_UMI_HDR_VALID | 0xFFFFu)) { printf("array: %zu records\n", n); bad++; }
    printf("%d mismatches\n", bad);
    return bad ? 1 : 0;
}
#endif
