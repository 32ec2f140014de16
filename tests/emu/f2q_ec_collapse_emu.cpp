// tests/emu/f2q_ec_collapse_emu.cpp -- TEST INFRASTRUCTURE.  The per-lane logic of f2q_ec_collapse (ec64_find, ecc_probe,
// ecc_parent_lane, ecc_root_lane of 2fast2q_amd/csrc/f2q_device.h: what k_ec_parent / k_ec_parent_lane / k_ec_roots run
// per lane) compiled with g++ and run over a single-word table filled from a key -> reads list, so the CPU suite can check
// it against the plain-Python rule (tests/ec_collapse_cases.py).  The product never uses this file.
#include "f2q_emu.cpp"

// k_ec_parent's round for one key on the host: lane n0 of a group of gsz lanes probes neighbours n0, n0 + 64, ...; the
// candidates are then reduced by the kernel's shuffle tree (lane i takes from lane i + off while that lane is in the group)
static uint32_t wave_parent(const EcDev &ec, uint32_t s, uint32_t ratio, uint32_t lmax)
{
    const unsigned long long k = ec.k64_slots[s], c = ec.k64_count[s] + 1ull;
    const uint32_t per = 3u * lmax, gsz = per < 64u ? per : 64u, own = 3u * ecc_length(k);
    unsigned long long br[64], bsn[64];
    for (uint32_t n0 = 0; n0 < gsz; n0++) {
        EccCand best{0ull, 0u, 0u};
        for (uint32_t n = n0; n < own; n += 64u) ecc_probe(ec, k, c, ratio, n, best);
        br[n0] = best.reads; bsn[n0] = ((unsigned long long)best.n << 32) | best.slot;
    }
    for (uint32_t off = 1; off < 64u; off <<= 1) {
        unsigned long long nr[64], nsn[64];
        for (uint32_t n0 = 0; n0 < gsz; n0++) {
            nr[n0] = br[n0]; nsn[n0] = bsn[n0];
            if (n0 + off < gsz && (br[n0 + off] > br[n0] || (br[n0 + off] == br[n0] && br[n0 + off] != 0ull && bsn[n0 + off] < bsn[n0]))) {
                nr[n0] = br[n0 + off]; nsn[n0] = bsn[n0 + off];
            }
        }
        memcpy(br, nr, sizeof(unsigned long long) * gsz); memcpy(bsn, nsn, sizeof(unsigned long long) * gsz);
    }
    return br[0] ? (uint32_t)bsn[0] : s;
}

extern "C" {

// keys/offs/reads/n: the table (distinct keys, upper case).  A key with a single-word form (ec64_word: plain or with up to
// three 'N's) goes into a single-word table of 1 << bits slots, every other key is a byte-string entry: its own centroid.
// wave 0: ecc_parent_lane per slot; 1: the wave-cooperative round per key (lmax = the longest key of its 64 slots).
// centroid[i] = the index of key i's centroid in the input order, cluster[i], extra[4] as f2q_ec_collapse gives them.
// Returns 0, -1 when the table is too small, -2 on a bad root.
int ecemu_collapse(const char *keys, const uint32_t *offs, const int64_t *reads, uint32_t n, int bits, int dist, int ratio, int wave,
                   uint64_t *centroid, int64_t *cluster, int64_t *extra)
{
    const size_t slots = (size_t)1 << bits;
    std::vector<unsigned long long> ks(slots, ~0ull), kc(slots, 0), kf(slots, ~0ull), ctr(8, 0);
    EcDev ec{};
    ec.k64_slots = ks.data(); ec.k64_count = kc.data(); ec.k64_first = kf.data(); ec.k64_mask = (uint32_t)(slots - 1); ec.ctr = ctr.data();
    std::vector<uint32_t> slot_of(n, F2Q_ECC_NONE), key_of(slots, F2Q_ECC_NONE);
    uint32_t held = 0;
    for (uint32_t i = 0; i < n; i++) {
        const int len = (int)(offs[i + 1] - offs[i]);
        uint64_t codes = 0; uint32_t nmask = 0; bool regular = len <= F2Q_EC64_MAXLEN;
        for (int j = 0; regular && j < len; j++) {
            const uint8_t ch = (uint8_t)keys[offs[i] + j];
            uint32_t c = base_code(ch);
            if (c > 3u) { if (ch == (uint8_t)'N') { nmask |= 1u << j; c = 0; } else regular = false; }
            codes |= (uint64_t)(c & 3u) << (2 * j);
        }
        unsigned long long word = 0;
        if (!regular || !ec64_word(codes, nmask, len, word)) continue;
        if (++held > slots / 4 * 3) return -1;
        ec64_insert_word(ec, word, i);
        const uint32_t s = ec64_find(ec, word);
        if (s == F2Q_ECC_NONE) return -1;
        kc[s] = (unsigned long long)reads[i] - 1ull;            // (the count word holds n - 1)
        slot_of[i] = s; key_of[s] = i;
    }
    for (uint32_t i = 0; i < n; i++) { centroid[i] = i; cluster[i] = reads[i]; }
    for (int k = 0; k < 4; k++) extra[k] = 0;
    if (!dist) return 0;
    std::vector<uint32_t> parent(slots), root(slots);
    std::vector<unsigned long long> cl(slots + F2Q_ECC_CTR_WORDS, 0);
    for (size_t base = 0; base < slots; base += 64) {
        uint32_t lmax = 0;
        for (size_t s = base; s < base + 64 && s < slots; s++) lmax = std::max(lmax, ecc_length(ks[s]));
        for (size_t s = base; s < base + 64 && s < slots; s++) {
            if (wave && ecc_length(ks[s])) parent[s] = wave_parent(ec, (uint32_t)s, (uint32_t)ratio, lmax);
            else if (wave) parent[s] = (uint32_t)s;
            else ecc_parent_lane(ec, parent.data(), (uint32_t)ratio, (uint32_t)s);
        }
    }
    unsigned long long tot[F2Q_ECC_CTR_WORDS] = {0, 0, 0, 0};
    for (size_t s = 0; s < slots; s++) ecc_root_lane(ec, parent.data(), root.data(), cl.data(), (uint32_t)s, tot);
    for (int k = 0; k < 4; k++) extra[k] = (int64_t)tot[k];
    for (uint32_t i = 0; i < n; i++) {
        if (slot_of[i] == F2Q_ECC_NONE) continue;
        const uint32_t r = root[slot_of[i]];
        if (r >= slots || key_of[r] == F2Q_ECC_NONE) return -2;
        centroid[i] = key_of[r]; cluster[i] = (int64_t)cl[slot_of[i]];
    }
    return 0;
}

}
