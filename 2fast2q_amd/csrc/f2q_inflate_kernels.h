// f2q_inflate_kernels.h -- k_inflate_bgzf: BGZF members inflated on the device, one wave (a 64-thread workgroup) per member.
// The reference reads a compressed file with gzip.open (fast2q.py:566-578); f2q_reader.h does it on the host, this
// header does it for BGZF on the GPU (F2Q_DEVICE_INFLATE=1, f2q_text_from_bgzf).
//
// A BGZF member is an independent gzip stream of at most 64 KiB of text, so one member's output fits in LDS and no
// back-reference leaves it.  Per workgroup (about 74 KiB of LDS: two workgroups per CU):
//   out     64 KiB   the member's text; matches copy inside it, then it is stored with 16-byte stores
//   ring     2 KiB   compressed input: two halves, the next half waits in registers (pre[]) while this one is decoded
//   ltab     4 KiB   litlen table, 10-bit root; dtab 1 KiB: distance table, 8-bit root (also the code-length table)
//   crctab   1 KiB   CRC-32 table; plus code-length arrays, per-length counts and 64 per-lane CRC / newline slots
// Decoding is serial and wave-uniform: every lane holds the same bit buffer and takes the same branches.  Codes longer
// than the root are decoded from the canonical counts (first code per length, symbols sorted by length) instead of
// sub-tables: they are rare and it keeps the tables at a fixed size.  The tables are built wave-parallel: per-length
// counts (a lane per length), a serial prefix over 15 lengths, a lane per length placing its symbols, a lane per table
// entry.  Fixed-Huffman blocks build their tables the same way when they occur (no LDS is kept for them: they are the
// short members, the end marker among them).
//
// Damaged input never faults or hangs: every LDS and global index is bounded, reading past the payload end plus the
// 8 trailer bytes stops decoding, every loop is bounded by the payload size, and the stream must end exactly where the
// trailer begins.  The status of each member tells what went wrong (F2Q_INF_*).
//
// The decoder core is host/device code: with INF_LANE 0 and INF_STEP 1 every wave-parallel step is a plain loop over
// all lanes, so tests/emu/inflate_dev_fuzz.cpp runs the same source under the sanitizers.  Every device write is a
// plain C++ store.
#pragma once
#include <stdint.h>

#ifndef F2Q_HD
#ifdef __HIPCC__
#define F2Q_HD __host__ __device__ __forceinline__
#else
#define F2Q_HD inline
#endif
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define INF_LANE ((uint32_t)threadIdx.x)
#define INF_STEP 64u
// the workgroup is one wave, whose LDS operations complete in order: a compiler fence at wavefront scope is all a
// wave-parallel step needs.  (A workgroup barrier would also wait for the ring's prefetch loads still in flight.)
#define INF_SYNC() __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront")
#define INF_UNROLL _Pragma("unroll")
#else
#define INF_LANE 0u
#define INF_STEP 1u
#define INF_SYNC() ((void)0)
#define INF_UNROLL
#endif

namespace f2q {

enum : uint32_t {
    F2Q_INF_OK = 0,
    F2Q_INF_OVERRUN = 1,        // the stream reads past its payload (plus the 8 trailer bytes), or the member lies outside the buffer
    F2Q_INF_BAD_BLOCK = 2,      // block type 3, stored length check, too many length / distance codes, loop bound
    F2Q_INF_BAD_CODE = 3,       // over-subscribed / incomplete code lengths, an unused code, a bad repeat, no end-of-block code
    F2Q_INF_DIST_FAR = 4,       // a distance before the member's start
    F2Q_INF_OUT_OVERFLOW = 5,   // more than 64 KiB of output, or the text would leave its buffer
    F2Q_INF_ISIZE = 6,          // output length differs from the trailer's ISIZE
    F2Q_INF_CRC = 7,            // CRC-32 differs from the trailer's
    F2Q_INF_TRAILING = 8,       // bytes left between the end of the deflate stream and the trailer
    F2Q_INF_NOT_RUN = 0xFFu     // (host: the status words are preset to this)
};

// one member, as the host describes it: in[in_off, in_off + in_len) is the deflate payload, the 8 trailer bytes follow
struct BgzfMember { uint64_t in_off; uint32_t in_len, isize, crc, out_off; uint32_t pad[2]; };
// what the kernel reports: status, bytes produced, 1 + offset of the member's last '\n' (0: none), its last byte
struct BgzfResult { uint32_t status, produced, last_nl, last_byte; };

#define F2Q_INF_OUT_BYTES 65536u
#define F2Q_INF_RING_W 512u                      // input ring, 32-bit words (2 KiB)
#define F2Q_INF_HALF_W (F2Q_INF_RING_W / 2)
#define F2Q_INF_PRE (F2Q_INF_HALF_W / INF_STEP)  // words of the next half held by each lane
#define F2Q_INF_LROOT 10
#define F2Q_INF_DROOT 8

struct InflLds {
    uint32_t out32[F2Q_INF_OUT_BYTES / 4];
    uint32_t ring[F2Q_INF_RING_W];
    uint32_t ltab[1u << F2Q_INF_LROOT];
    uint32_t dtab[1u << F2Q_INF_DROOT];
    uint32_t crctab[256];
    uint32_t x2n[32];
    uint32_t lane_crc[64], lane_nl[64];
    uint16_t lsym[288], dsym[32];
    uint16_t lcnt[16], loffs[16], lfirst[16], dcnt[16], doffs[16], dfirst[16];
    uint8_t lens[320];
};

// table entry: bits 0-4 code length, 5-8 extra bits, 9-11 kind, 16-31 value (literal byte / length or distance base)
enum : uint32_t { INF_K_LIT = 0, INF_K_BASE = 1, INF_K_EOB = 2, INF_K_LONG = 3, INF_K_BAD = 4 };
enum : int { INF_T_LITLEN = 0, INF_T_DIST = 1, INF_T_CLEN = 2 };

F2Q_HD uint32_t inf_entry(uint32_t kind, uint32_t nbits, uint32_t extra, uint32_t val) { return nbits | (extra << 5) | (kind << 9) | (val << 16); }
F2Q_HD uint32_t inf_kind(uint32_t e) { return (e >> 9) & 7u; }

// the entry of symbol s of a table of type t, coded with len bits (RFC 1951 3.2.5)
F2Q_HD uint32_t inf_sym_entry(int t, uint32_t s, uint32_t len)
{
    if (t == INF_T_CLEN) return inf_entry(INF_K_LIT, len, 0, s);
    if (t == INF_T_DIST) {
        if (s < 4) return inf_entry(INF_K_BASE, len, 0, 1 + s);
        if (s < 30) { const uint32_t e = (s - 2) >> 1; return inf_entry(INF_K_BASE, len, e, ((2u + (s & 1u)) << e) + 1u); }
        return inf_entry(INF_K_BAD, len, 0, 0);
    }
    if (s < 256) return inf_entry(INF_K_LIT, len, 0, s);
    if (s == 256) return inf_entry(INF_K_EOB, len, 0, 0);
    const uint32_t k = s - 257;
    if (k < 8) return inf_entry(INF_K_BASE, len, 0, 3 + k);
    if (k < 28) { const uint32_t e = (k - 4) >> 2; return inf_entry(INF_K_BASE, len, e, ((4u + (k & 3u)) << e) + 3u); }
    if (k == 28) return inf_entry(INF_K_BASE, len, 0, 258);
    return inf_entry(INF_K_BAD, len, 0, 0);
}

F2Q_HD uint32_t inf_rev(uint32_t v, int n)
{
    uint32_t r = 0;
    for (int i = 0; i < n; i++) { r = (r << 1) | (v & 1u); v >>= 1; }
    return r;
}

// Canonical Huffman table of n code lengths (lens, in LDS), primary table of 2^ROOT entries.  Longer codes get a LONG
// entry and are finished by inf_decode_long from cnt / first / offs / sym.  codes: the code-length code (an incomplete
// set is never allowed); otherwise an incomplete set is allowed only for a single code of length 1, as zlib does.
template <int ROOT>
F2Q_HD uint32_t inf_build(const uint8_t *lens, uint32_t n, uint32_t *tab, uint16_t *cnt, uint16_t *offs, uint16_t *first, uint16_t *sym,
                          int type)
{
    for (uint32_t L = INF_LANE; L < 16; L += INF_STEP) {
        uint32_t k = 0;
        for (uint32_t s = 0; s < n; s++) k += lens[s] == L;
        cnt[L] = (uint16_t)(L ? k : 0);
    }
    INF_SYNC();
    int left = 1;
    uint32_t maxlen = 0, code = 0, o = 0;
    for (uint32_t L = 1; L < 16; L++) {
        const uint32_t c = cnt[L];
        left = left * 2 - (int)c;
        if (c) maxlen = L;
        if (left < 0) break;
        code = (code + (L > 1 ? cnt[L - 1] : 0u)) << 1;
        if (INF_LANE == 0) { first[L] = (uint16_t)code; offs[L] = (uint16_t)o; }
        o += c;
    }
    if (maxlen && (left < 0 || (left > 0 && (type == INF_T_CLEN || maxlen != 1)))) { INF_SYNC(); return F2Q_INF_BAD_CODE; }
    INF_SYNC();
    for (uint32_t L = INF_LANE + 1; L < 16; L += INF_STEP) {
        uint32_t k = offs[L];
        for (uint32_t s = 0; s < n; s++)
            if (lens[s] == L) sym[k++] = (uint16_t)s;
    }
    INF_SYNC();
    for (uint32_t i = INF_LANE; i < (1u << ROOT); i += INF_STEP) {
        const uint32_t c = inf_rev(i, ROOT);
        uint32_t e = inf_entry(INF_K_LONG, 0, 0, 0);
        for (uint32_t L = 1; L <= (uint32_t)ROOT; L++) {
            const uint32_t d = (c >> (ROOT - L)) - first[L];
            if (d < cnt[L]) { e = inf_sym_entry(type, sym[offs[L] + d], L); break; }
        }
        tab[i] = e;
    }
    INF_SYNC();
    return F2Q_INF_OK;
}

// a code longer than the root: one bit at a time against the canonical first code of each length
F2Q_HD uint32_t inf_decode_long(uint64_t bb, int root, const uint16_t *cnt, const uint16_t *offs, const uint16_t *first, const uint16_t *sym, int type)
{
    uint32_t code = inf_rev((uint32_t)bb & ((1u << root) - 1u), root);
    for (int L = root + 1; L < 16; L++) {
        code = (code << 1) | (uint32_t)((bb >> (L - 1)) & 1u);
        const uint32_t d = code - first[L];
        if (cnt[L] && d < cnt[L]) return inf_sym_entry(type, sym[offs[L] + d], (uint32_t)L);
    }
    return inf_entry(INF_K_BAD, 0, 0, 0);
}

// ---- CRC-32 (zlib's polynomial; combine as crc32_combine: multiply by x^(8 len) mod P) -------------------------------
#define F2Q_INF_POLY 0xedb88320u
F2Q_HD uint32_t inf_multmodp(uint32_t a, uint32_t b)
{
    uint32_t m = 1u << 31, p = 0;
    for (int i = 0; i < 32; i++) {
        if (a & m) p ^= b;
        m >>= 1;
        b = (b & 1u) ? (b >> 1) ^ F2Q_INF_POLY : b >> 1;
    }
    return p;
}
F2Q_HD uint32_t inf_x8n(const uint32_t *x2n, uint32_t n)
{
    uint32_t p = 1u << 31, k = 3;
    while (n) { if (n & 1u) p = inf_multmodp(x2n[k & 31u], p); n >>= 1; k++; }
    return p;
}

// once per workgroup: CRC table and x^(2^k) mod P
F2Q_HD void inf_wg_init(InflLds &S)
{
    for (uint32_t i = INF_LANE; i < 256; i += INF_STEP) {
        uint32_t c = i;
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ F2Q_INF_POLY : c >> 1;
        S.crctab[i] = c;
    }
    if (INF_LANE == 0) {
        uint32_t p = 1u << 30;
        S.x2n[0] = p;
        for (int k = 1; k < 32; k++) S.x2n[k] = p = inf_multmodp(p, p);
    }
    INF_SYNC();
}

// compressed input word w of the 4-byte aligned buffer `in`, the address clamped to the word that holds byte lim - 1;
// inf_in_mask then zeroes the bytes at or past lim.  Kept apart so that a prefetched word is not used (waited for) until
// it goes into the ring.
F2Q_HD uint32_t inf_in_load(const uint8_t *in, uint64_t w, uint64_t lim)
{
    const uint64_t last = (lim - 1) >> 2;
    return ((const uint32_t *)in)[w < last ? w : last];
}
F2Q_HD uint32_t inf_in_mask(uint32_t v, uint64_t w, uint64_t lim)
{
    if (w * 4 >= lim) return 0;
    if (w * 4 + 4 > lim) v &= (1u << (8 * (uint32_t)(lim - w * 4))) - 1u;
    return v;
}

// Inflate one member into S.out32.  in must be 4-byte aligned and readable up to the next multiple of 4 past the
// member's end; in_cap bytes of it belong to the caller's buffer.  Returns F2Q_INF_* and fills r.
F2Q_HD uint32_t inf_member(InflLds &S, const uint8_t *in, uint64_t in_cap, const BgzfMember &m, BgzfResult &r)
{
    uint8_t *out = (uint8_t *)S.out32;
    r.status = F2Q_INF_OK; r.produced = 0; r.last_nl = 0; r.last_byte = 0;
    const uint64_t q0 = m.in_off, pend = q0 + m.in_len, lim = pend + 8;
    if (lim > in_cap || lim < q0) { r.status = F2Q_INF_OVERRUN; return r.status; }
    if (m.isize > F2Q_INF_OUT_BYTES) { r.status = F2Q_INF_OUT_OVERFLOW; return r.status; }
    const uint32_t cap = m.isize;
    uint32_t st = F2Q_INF_OK, p = 0;
    uint32_t budget = 8u * (m.in_len + 16u) + 64u;    // every step consumes at least one bit
    // input ring: words [hi - RING_W, hi) are in S.ring, words [hi, hi + HALF_W) in pre[] (lane-strided)
    uint32_t pre[F2Q_INF_PRE];
    uint64_t hi = 0;
    auto ring_reset = [&](uint64_t q) {
        const uint64_t w0 = q >> 2;
        INF_SYNC();
        for (uint32_t i = INF_LANE; i < F2Q_INF_RING_W; i += INF_STEP) S.ring[(w0 + i) & (F2Q_INF_RING_W - 1)] = inf_in_mask(inf_in_load(in, w0 + i, lim), w0 + i, lim);
        hi = w0 + F2Q_INF_RING_W;
        INF_UNROLL for (uint32_t k = 0; k < F2Q_INF_PRE; k++) pre[k] = inf_in_load(in, hi + INF_LANE + k * INF_STEP, lim);
        INF_SYNC();
    };
    auto ring_advance = [&]() {
        INF_SYNC();
        INF_UNROLL for (uint32_t k = 0; k < F2Q_INF_PRE; k++) { const uint64_t w = hi + INF_LANE + k * INF_STEP; S.ring[w & (F2Q_INF_RING_W - 1)] = inf_in_mask(pre[k], w, lim); }
        hi += F2Q_INF_HALF_W;
        INF_UNROLL for (uint32_t k = 0; k < F2Q_INF_PRE; k++) pre[k] = inf_in_load(in, hi + INF_LANE + k * INF_STEP, lim);
        INF_SYNC();
    };
    uint64_t bb = 0, ip = q0;
    uint32_t bc = 0;
    ring_reset(q0);
    // at least 32 bits in bb afterwards, unless the stream has run past its end
    auto refill = [&]() -> bool {
        if (bc > 32) return true;
        const uint64_t w = ip >> 2;
        if (w + 1 >= hi + F2Q_INF_HALF_W || w + F2Q_INF_RING_W < hi) ring_reset(ip);
        else if (w + 1 >= hi) ring_advance();
        const uint64_t v2 = ((uint64_t)S.ring[(w + 1) & (F2Q_INF_RING_W - 1)] << 32) | S.ring[w & (F2Q_INF_RING_W - 1)];
        bb |= (uint64_t)(uint32_t)(v2 >> (8 * (ip & 3))) << bc;
        bc += 32; ip += 4;
        if (ip > lim) { st = F2Q_INF_OVERRUN; return false; }
        return true;
    };
    auto bits = [&](uint32_t n) -> uint32_t { const uint32_t v = (uint32_t)bb & ((1u << n) - 1u); bb >>= n; bc -= n; return v; };
    auto room = [&](uint32_t n) -> bool {
        if (p + n <= cap) return true;
        st = p + n > F2Q_INF_OUT_BYTES ? F2Q_INF_OUT_OVERFLOW : F2Q_INF_ISIZE;
        return false;
    };

    bool last = false;
    while (!last && st == F2Q_INF_OK) {
        if (!budget--) { st = F2Q_INF_BAD_BLOCK; break; }
        if (!refill()) break;
        last = bits(1) != 0;
        const uint32_t type = bits(2);
        if (type == 0) {                                       // stored: a wave-wide copy from global memory
            bits(bc & 7u);
            uint64_t q = ip - (bc >> 3);
            bb = 0; bc = 0;
            if (q + 4 > pend) { st = F2Q_INF_OVERRUN; break; }
            const uint32_t len = in[q] | ((uint32_t)in[q + 1] << 8), nlen = in[q + 2] | ((uint32_t)in[q + 3] << 8);
            q += 4;
            if (len != (~nlen & 0xFFFFu)) { st = F2Q_INF_BAD_BLOCK; break; }
            if (q + len > pend) { st = F2Q_INF_OVERRUN; break; }
            if (!room(len)) break;
            for (uint32_t i = INF_LANE; i < len; i += INF_STEP) out[p + i] = in[q + i];
            INF_SYNC();
            p += len; ip = q + len;
            continue;
        }
        if (type == 3) { st = F2Q_INF_BAD_BLOCK; break; }
        uint32_t nlen = 288, ndist = 32;
        if (type == 1) {                                       // fixed Huffman codes (RFC 1951 3.2.6)
            for (uint32_t i = INF_LANE; i < 320; i += INF_STEP) S.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
            INF_SYNC();
        } else {                                               // dynamic: code-length code, then the two code lengths
            if (!refill()) break;
            nlen = bits(5) + 257; ndist = bits(5) + 1;
            const uint32_t ncl = bits(4) + 4;
            if (nlen > 286 || ndist > 30) { st = F2Q_INF_BAD_BLOCK; break; }
            if (!refill()) break;
            uint64_t cl = bits(ncl > 10 ? 30 : 3 * ncl);
            if (ncl > 10) { if (!refill()) break; cl |= (uint64_t)bits(3 * (ncl - 10)) << 30; }
            for (uint32_t s = INF_LANE; s < 19; s += INF_STEP) {
                // position of symbol s in the transmitted order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
                const uint32_t j = s >= 16 ? s - 16 : s == 0 ? 3 : s < 8 ? 19 - 2 * s : 2 * s - 12;
                S.lens[s] = (uint8_t)(j < ncl ? (cl >> (3 * j)) & 7u : 0u);
            }
            INF_SYNC();
            if ((st = inf_build<7>(S.lens, 19, S.dtab, S.dcnt, S.doffs, S.dfirst, S.dsym, INF_T_CLEN)) != F2Q_INF_OK) break;
            const uint32_t total = nlen + ndist;
            uint32_t i = 0, prev = 0;
            while (i < total) {
                if (!budget--) { st = F2Q_INF_BAD_BLOCK; break; }
                if (!refill()) break;
                const uint32_t e = S.dtab[bb & 127u];
                if (inf_kind(e) != INF_K_LIT) { st = F2Q_INF_BAD_CODE; break; }
                bits(e & 31u);
                const uint32_t sym = e >> 16;
                if (sym < 16) {
                    if (INF_LANE == 0) S.lens[i] = (uint8_t)sym;
                    i++; prev = sym;
                    continue;
                }
                uint32_t rep, v = 0;
                if (sym == 16) { if (i == 0) { st = F2Q_INF_BAD_CODE; break; } rep = 3 + bits(2); v = prev; }
                else if (sym == 17) rep = 3 + bits(3);
                else rep = 11 + bits(7);
                if (i + rep > total) { st = F2Q_INF_BAD_CODE; break; }
                for (uint32_t k = INF_LANE; k < rep; k += INF_STEP) S.lens[i + k] = (uint8_t)v;
                i += rep; prev = v;
            }
            INF_SYNC();
            if (st != F2Q_INF_OK) break;
            if (S.lens[256] == 0) { st = F2Q_INF_BAD_CODE; break; }          // no end-of-block code
        }
        if ((st = inf_build<F2Q_INF_LROOT>(S.lens, nlen, S.ltab, S.lcnt, S.loffs, S.lfirst, S.lsym, INF_T_LITLEN)) != F2Q_INF_OK) break;
        if ((st = inf_build<F2Q_INF_DROOT>(S.lens + (type == 1 ? 288 : nlen), ndist, S.dtab, S.dcnt, S.doffs, S.dfirst, S.dsym, INF_T_DIST)) != F2Q_INF_OK) break;
        for (;;) {                                             // the symbols of one block
            if (!budget--) { st = F2Q_INF_BAD_BLOCK; break; }
            if (!refill()) break;
            uint32_t e = S.ltab[bb & ((1u << F2Q_INF_LROOT) - 1u)];
            if (inf_kind(e) == INF_K_LONG) e = inf_decode_long(bb, F2Q_INF_LROOT, S.lcnt, S.loffs, S.lfirst, S.lsym, INF_T_LITLEN);
            const uint32_t kind = inf_kind(e);
            if (kind == INF_K_LIT) {
                bits(e & 31u);
                if (!room(1)) break;
                if (INF_LANE == 0) out[p] = (uint8_t)(e >> 16);
                p++;
                continue;
            }
            if (kind == INF_K_EOB) { bits(e & 31u); break; }
            if (kind != INF_K_BASE) { st = F2Q_INF_BAD_CODE; break; }
            bits(e & 31u);
            const uint32_t len = (e >> 16) + bits((e >> 5) & 15u);
            if (!refill()) break;
            uint32_t de = S.dtab[bb & ((1u << F2Q_INF_DROOT) - 1u)];
            if (inf_kind(de) == INF_K_LONG) de = inf_decode_long(bb, F2Q_INF_DROOT, S.dcnt, S.doffs, S.dfirst, S.dsym, INF_T_DIST);
            if (inf_kind(de) != INF_K_BASE) { st = F2Q_INF_BAD_CODE; break; }
            bits(de & 31u);
            const uint32_t d = (de >> 16) + bits((de >> 5) & 15u);
            if (d > p) { st = F2Q_INF_DIST_FAR; break; }
            if (!room(len)) break;
            // out[p + i] = out[p - d + (i mod d)]: right for overlapping matches too; one wave's LDS operations complete in order
            if (d >= len) { for (uint32_t k = INF_LANE; k < len; k += INF_STEP) out[p + k] = out[p - d + k]; }
            else { for (uint32_t k = INF_LANE; k < len; k += INF_STEP) out[p + k] = out[p - d + k % d]; }
            p += len;
        }
        INF_SYNC();
    }
    r.produced = p;
    if (st == F2Q_INF_OK) {
        const uint64_t end = (ip * 8 - bc + 7) / 8;          // the stream ends at a byte boundary
        if (end > pend) st = F2Q_INF_OVERRUN;
        else if (end < pend) st = F2Q_INF_TRAILING;
        else if (p != m.isize) st = F2Q_INF_ISIZE;
    }
    if (st == F2Q_INF_OK) {                                    // CRC-32: a slice per lane, combined in lane order
        const uint32_t sl = (p + 63) / 64;
        for (uint32_t j = INF_LANE; j < 64; j += INF_STEP) {
            const uint32_t a = j * sl < p ? j * sl : p, b = a + sl < p ? a + sl : p;
            uint32_t c = 0xFFFFFFFFu, nl = 0;
            for (uint32_t k = a; k < b; k++) {
                const uint32_t ch = out[k];
                c = S.crctab[(c ^ ch) & 0xFFu] ^ (c >> 8);
                if (ch == 0x0a) nl = k + 1;
            }
            S.lane_crc[j] = c ^ 0xFFFFFFFFu; S.lane_nl[j] = nl;
        }
        INF_SYNC();
        const uint32_t xs = inf_x8n(S.x2n, sl);
        uint32_t crc = 0, nl = 0;
        for (uint32_t j = 0; j < 64; j++) {
            const uint32_t a = j * sl < p ? j * sl : p, b = a + sl < p ? a + sl : p;
            if (b > a) crc = inf_multmodp(b - a == sl ? xs : inf_x8n(S.x2n, b - a), crc) ^ S.lane_crc[j];
            nl = S.lane_nl[j] > nl ? S.lane_nl[j] : nl;
        }
        if (crc != m.crc) st = F2Q_INF_CRC;
        r.last_nl = nl; r.last_byte = p ? out[p - 1] : 0;
    }
    INF_SYNC();
    r.status = st;
    return st;
}

#if defined(__HIPCC__)
// members mem[0, n) of the compressed buffer `in` (in_cap bytes) -> text + out_off (text_cap bytes); res[i] per member.
// A member whose status is not OK writes no text.  Grid-stride over the members, 64 threads per workgroup.
__global__ __launch_bounds__(64) void k_inflate_bgzf(const uint8_t *in, uint64_t in_cap, const BgzfMember *mem, uint32_t n, uint8_t *text,
                                                     uint64_t text_cap, BgzfResult *res)
{
    __shared__ InflLds S;
    inf_wg_init(S);
    for (uint32_t mi = blockIdx.x; mi < n; mi += gridDim.x) {
        const BgzfMember m = mem[mi];
        BgzfResult r;
        uint32_t st;
        if ((uint64_t)m.out_off + m.isize > text_cap) { r.status = st = F2Q_INF_OUT_OVERFLOW; r.produced = r.last_nl = r.last_byte = 0; }
        else st = inf_member(S, in, in_cap, m, r);
        if (st == F2Q_INF_OK && m.isize) {
            // text + out_off: bytes up to a 16-byte boundary, then 16-byte stores, then the tail
            uint8_t *dst = text + m.out_off;
            const uint8_t *ob = (const uint8_t *)S.out32;
            const uint32_t mis = (uint32_t)((uintptr_t)dst & 15u), head = mis ? (16u - mis < m.isize ? 16u - mis : m.isize) : 0u;
            const uint32_t nv = (m.isize - head) / 16u, tail0 = head + nv * 16u;
            if (threadIdx.x < head) dst[threadIdx.x] = ob[threadIdx.x];
            const uint32_t sh = (head & 3u) * 8u;
            for (uint32_t v = threadIdx.x; v < nv; v += 64) {
                const uint32_t w = (head + v * 16u) >> 2;
                uint32_t x[5];
#pragma unroll
                for (int k = 0; k < 4; k++) x[k] = S.out32[w + k];
                x[4] = sh ? S.out32[w + 4 < F2Q_INF_OUT_BYTES / 4 ? w + 4 : F2Q_INF_OUT_BYTES / 4 - 1] : 0u;
                uint4 o;
                o.x = sh ? (x[0] >> sh) | (x[1] << (32 - sh)) : x[0];
                o.y = sh ? (x[1] >> sh) | (x[2] << (32 - sh)) : x[1];
                o.z = sh ? (x[2] >> sh) | (x[3] << (32 - sh)) : x[2];
                o.w = sh ? (x[3] >> sh) | (x[4] << (32 - sh)) : x[3];
                *(uint4 *)(dst + head + v * 16u) = o;
            }
            for (uint32_t k = tail0 + threadIdx.x; k < m.isize; k += 64) dst[k] = ob[k];
        }
        if (threadIdx.x == 0) res[mi] = r;
        __syncthreads();
    }
}
#endif

}  // namespace f2q
