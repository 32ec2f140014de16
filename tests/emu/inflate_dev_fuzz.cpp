// Checker for the decoder core of k_inflate_bgzf (2fast2q_amd/csrc/f2q_inflate_kernels.h), compiled for the host: the
// wave-parallel steps run as loops over all lanes.  Build with -fsanitize=address,undefined.
//
//   inflate_dev_fuzz corpus              every kind of payload x zlib levels 0 1 6 9 x strategies, empty members and
//                                        members of exactly 65536 bytes: status OK, bytes equal to the input
//   inflate_dev_fuzz fuzz <n> [seed]     n damaged members (bit flips, cut-offs, flipped trailers): the core agrees
//                                        with zlib on accept / reject (an accepted copy has the same bytes)
//   inflate_dev_fuzz file <path> [seed]  records of <u32 member bytes><payload><crc><isize>: prints one status per line
//   inflate_dev_fuzz bytes <path> <seed> <out>   the same, and writes a record <u32 text bytes><text> per member to <out>
//                                        (no text unless the status is OK).  With a seed, every payload starts at an
//                                        offset = seed mod 4 of its block: seeds 0..3 meet every alignment
//
// Every member is placed at a random offset of a 4-byte aligned heap block that ends 4 bytes (rounded up) past the
// trailer, so ASan sees any read outside what the kernel may read.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <string>
#include <vector>

#include "../../2fast2q_amd/csrc/f2q_inflate_kernels.h"

using namespace f2q;

static uint64_t rs = 88172645463325252ull;
static uint32_t rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (uint32_t)(rs >> 11); }
static InflLds *S;
static int in_res = -1;      // file / bytes: every member's payload starts at an offset = in_res mod 4 (the seed mod 4)

static std::vector<uint8_t> make(int kind, size_t n)
{
    std::vector<uint8_t> d(n);
    switch (kind) {
    case 0: for (auto &c : d) c = (uint8_t)rnd(); break;                                          // random bytes
    case 1: {                                                                                     // synthetic FASTQ
        size_t i = 0; uint32_t r = 0;
        while (i < n) {
            std::string rec = "@read" + std::to_string(r++) + "\n";
            const int L = 50 + rnd() % 120;
            for (int k = 0; k < L; k++) rec += "ACGT"[rnd() & 3];
            rec += "\n+\n";
            for (int k = 0; k < L; k++) rec += (char)(rnd() % 8 ? 'F' : '!' + rnd() % 40);
            rec += "\n";
            for (size_t k = 0; k < rec.size() && i < n; k++) d[i++] = (uint8_t)rec[k];
        }
    } break;
    case 2: for (auto &c : d) c = 'A'; break;                                                      // distance-1 runs, 258-byte matches
    case 3: for (size_t i = 0; i < n; i++) d[i] = (uint8_t)"ACGTTGCA"[i % 8]; break;               // period 8
    case 4: { size_t i = 0; while (i < n) { size_t L = 1 + rnd() % 300, back = i ? 1 + rnd() % (i < 40000 ? i : 40000) : 0; for (size_t j = 0; j < L && i < n; j++, i++) d[i] = (back && (rnd() & 7)) ? d[i - back] : (uint8_t)rnd(); } } break;
    default: for (size_t i = 0; i < n; i++) d[i] = (uint8_t)(i % 5 == 0 ? rnd() : 'I'); break;
    }
    return d;
}

static std::vector<uint8_t> deflate_raw(const std::vector<uint8_t> &d, int level, int strat)
{
    std::vector<uint8_t> c(d.size() + d.size() / 8 + 1024);
    z_stream zs = {};
    if (deflateInit2(&zs, level, Z_DEFLATED, -15, 8, strat) != Z_OK) { printf("deflateInit2 failed\n"); exit(1); }
    zs.next_in = const_cast<uint8_t *>(d.data()); zs.avail_in = (uInt)d.size(); zs.next_out = c.data(); zs.avail_out = (uInt)c.size();
    if (deflate(&zs, Z_FINISH) != Z_STREAM_END) { printf("deflate failed\n"); exit(1); }
    c.resize(zs.total_out);
    deflateEnd(&zs);
    return c;
}

static void put32(std::vector<uint8_t> &v, uint32_t x) { for (int k = 0; k < 4; k++) v.push_back((uint8_t)(x >> (8 * k))); }

// payload followed by its trailer (crc, isize) -> status of the core; the text in *out
static uint32_t run(const std::vector<uint8_t> &member, std::vector<uint8_t> *out)
{
    if (member.size() < 8) return F2Q_INF_OVERRUN;
    const size_t off = in_res < 0 ? rnd() % 16 : in_res + 4 * (rnd() % 4), end = off + member.size(), words = (end + 3) / 4;
    uint32_t *blk = (uint32_t *)malloc(words * 4);
    uint8_t *b = (uint8_t *)blk;
    for (size_t i = 0; i < words * 4; i++) b[i] = (uint8_t)rnd();                  // garbage around the member
    memcpy(b + off, member.data(), member.size());
    BgzfMember m = {};
    m.in_off = off; m.in_len = (uint32_t)(member.size() - 8);
    const uint8_t *t = member.data() + member.size() - 8;
    m.crc = t[0] | (t[1] << 8) | (t[2] << 16) | ((uint32_t)t[3] << 24);
    m.isize = t[4] | (t[5] << 8) | (t[6] << 16) | ((uint32_t)t[7] << 24);
    BgzfResult r;
    const uint32_t st = inf_member(*S, b, end, m, r);
    if (st != r.status) { printf("status word %u differs from the returned %u\n", r.status, st); exit(1); }
    if (st == F2Q_INF_OK && out) out->assign((uint8_t *)S->out32, (uint8_t *)S->out32 + r.produced);
    if (st == F2Q_INF_OK) {                                                            // the newline / last byte report
        uint32_t nl = 0;
        for (uint32_t i = 0; i < r.produced; i++) if (((uint8_t *)S->out32)[i] == '\n') nl = i + 1;
        if (nl != r.last_nl || r.last_byte != (r.produced ? ((uint8_t *)S->out32)[r.produced - 1] : 0u)) { printf("last_nl / last_byte wrong\n"); exit(1); }
    }
    free(blk);
    return st;
}

// zlib's verdict on the same member: inflate must end exactly at the trailer, CRC and ISIZE must match
static bool zlib_ok(const std::vector<uint8_t> &member, std::vector<uint8_t> &out)
{
    if (member.size() < 8) return false;
    const size_t in_len = member.size() - 8;
    out.assign(65536 + 1, 0);
    z_stream zs = {};
    if (inflateInit2(&zs, -15) != Z_OK) return false;
    zs.next_in = const_cast<uint8_t *>(member.data()); zs.avail_in = (uInt)in_len; zs.next_out = out.data(); zs.avail_out = (uInt)out.size();
    const int r = inflate(&zs, Z_FINISH);
    const bool ended = r == Z_STREAM_END && zs.avail_in == 0;
    out.resize(zs.total_out);
    inflateEnd(&zs);
    const uint8_t *t = member.data() + in_len;
    const uint32_t crc = t[0] | (t[1] << 8) | (t[2] << 16) | ((uint32_t)t[3] << 24), isz = t[4] | (t[5] << 8) | (t[6] << 16) | ((uint32_t)t[7] << 24);
    return ended && out.size() <= 65536 && isz == out.size() && crc == (uint32_t)crc32(0, out.data(), (uInt)out.size());
}

static std::vector<uint8_t> member_of(const std::vector<uint8_t> &d, int level, int strat)
{
    std::vector<uint8_t> m = deflate_raw(d, level, strat);
    put32(m, (uint32_t)crc32(0, d.data(), (uInt)d.size()));
    put32(m, (uint32_t)d.size());
    return m;
}

static const int STRATS[] = {Z_DEFAULT_STRATEGY, Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE, Z_FILTERED};

static int corpus()
{
    long n = 0;
    const int levels[] = {0, 1, 6, 9};
    const size_t sizes[] = {0, 1, 100, 4093, 30000, 65280, 65535, 65536};
    for (int kind = 0; kind < 6; kind++)
        for (size_t sz : sizes)
            for (int lv : levels)
                for (int strat : STRATS) {
                    if (lv == 0 && strat != Z_DEFAULT_STRATEGY) continue;
                    const std::vector<uint8_t> d = make(kind, sz);
                    std::vector<uint8_t> out;
                    const uint32_t st = run(member_of(d, lv, strat), &out);
                    if (st != F2Q_INF_OK || out != d) { printf("corpus MISMATCH kind %d size %zu level %d strategy %d status %u\n", kind, sz, lv, strat, st); return 1; }
                    n++;
                }
    printf("ok %ld members\n", n);
    return 0;
}

static int fuzz(int iters)
{
    long rej = 0, acc = 0;
    for (int it = 0; it < iters; it++) {
        const int kind = rnd() % 6, lv = (int[]){0, 1, 6, 9}[rnd() % 4], strat = STRATS[rnd() % 5];
        const size_t sz = rnd() % 4 == 0 ? 65536 : rnd() % 8 == 0 ? rnd() % 8 : rnd() % 20000;
        const std::vector<uint8_t> d = make(kind, sz);
        std::vector<uint8_t> m = member_of(d, lv, strat);
        const uint32_t how = rnd() % 8;
        if (how < 4) { const size_t bit = rnd() % (m.size() * 8); m[bit / 8] ^= (uint8_t)(1u << (bit % 8)); }
        else if (how < 6) {                                                            // cut the payload, keep the trailer
            const size_t keep = m.size() > 8 ? rnd() % (m.size() - 8) : 0;
            std::vector<uint8_t> t(m.end() - 8, m.end());
            m.resize(keep); m.insert(m.end(), t.begin(), t.end());
        } else if (how == 6) { for (int k = 0; k < 1 + (int)(rnd() % 4); k++) { const size_t p = rnd() % m.size(); m[p] = (uint8_t)rnd(); } }
        else m.insert(m.end() - 8, (uint8_t)rnd());                                     // a byte left before the trailer
        std::vector<uint8_t> zo, o;
        const bool zok = zlib_ok(m, zo);
        const uint32_t st = run(m, &o);
        if (zok != (st == F2Q_INF_OK) || (zok && o != zo)) { printf("fuzz iter %d DISAGREES: zlib %d core %u (how %u kind %d size %zu level %d strategy %d)\n", it, zok, st, how, kind, sz, lv, strat); return 1; }
        (zok ? acc : rej)++;
    }
    printf("ok %d damaged members, %ld rejected, %ld accepted by both\n", iters, rej, acc);
    return 0;
}

static int file(const char *path, const char *text_path)
{
    FILE *f = fopen(path, "rb"), *o = text_path ? fopen(text_path, "wb") : nullptr;
    if (!f || (text_path && !o)) { printf("cannot open %s\n", f ? text_path : path); return 1; }
    uint8_t h[4];
    while (fread(h, 1, 4, f) == 4) {
        const uint32_t n = h[0] | (h[1] << 8) | (h[2] << 16) | ((uint32_t)h[3] << 24);
        std::vector<uint8_t> m(n), out;
        if (n && fread(m.data(), 1, n, f) != n) { printf("short record\n"); return 1; }
        printf("%u\n", run(m, &out));
        if (o) {
            std::vector<uint8_t> len;
            put32(len, (uint32_t)out.size());
            if (fwrite(len.data(), 1, 4, o) != 4 || (out.size() && fwrite(out.data(), 1, out.size(), o) != out.size())) { printf("cannot write %s\n", text_path); return 1; }
        }
    }
    fclose(f);
    if (o) fclose(o);
    return 0;
}

int main(int argc, char **argv)
{
    S = new InflLds();
    inf_wg_init(*S);
    if (argc > 3) rs ^= (uint64_t)atoll(argv[3]) * 0x9E3779B97F4A7C15ull;
    const std::string mode = argc > 1 ? argv[1] : "corpus";
    int rc = 1;
    if ((mode == "file" || mode == "bytes") && argc > 3) in_res = atoi(argv[3]) & 3;
    if (mode == "corpus") rc = corpus();
    else if (mode == "fuzz") rc = fuzz(argc > 2 ? atoi(argv[2]) : 1000);
    else if (mode == "file" && argc > 2) rc = file(argv[2], nullptr);
    else if (mode == "bytes" && argc > 4) rc = file(argv[2], argv[4]);
    delete S;
    return rc;
}
