// tests/emu/lt_split.cpp -- TEST INFRASTRUCTURE.  Host build of k_count_fixed4_lds's two-stage decision
// (f2q_device.h: lt_probe0 / lt_exact_stage, the batch records and the compaction helpers), checked read by read
// against the one-stage decision it replaces (lt_probe + lt_decide on every read).  Used by test_lt_split_cpu.py.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../2fast2q_amd/csrc/f2q_device.h"
#include "../../2fast2q_amd/csrc/f2q_host.h"

using namespace f2q;

namespace {
template <bool NEAR>
LtVerdict decide(const LtDesc &lt, uint64_t key, uint32_t forced)
{
    const LtProbe q = lt_probe(lt, key);
    U2 e[4];
    for (int k = 0; k < 4; k++) {
        const uint32_t *tb = lt.tags + (size_t)(k >> 1) * F2Q_LT_SLOTS + 2u * q.b[k];
        e[k] = NEAR || k < 2 ? U2{tb[0], tb[1]} : U2{F2Q_LT_EMPTY, F2Q_LT_EMPTY};
    }
    auto rd0 = [&](uint32_t bk) { return U2{lt.tags[2u * bk], lt.tags[2u * bk + 1u]}; };
    return lt_decide<NEAR>(lt, q, e, forced, rd0);
}

template <bool NEAR>
void run(const LtDesc &lt, const uint64_t *keys, const uint32_t *forced_in, const uint8_t *cand_in, uint32_t n, uint64_t *out)
{
    for (uint32_t i = 0; i < n; i++) {
        const bool cand = cand_in[i] != 0;
        const uint32_t forced = cand ? forced_in[i] : 0u;          // the kernel reads the flags of candidates only
        const uint64_t key = keys[i];
        // one stage (the kernel before the split): every read through lt_decide, counted when it is a candidate
        const LtVerdict r = decide<NEAR>(lt, key, forced);
        const int ref = !cand ? 0 : r.perfect ? 1 : r.imperfect ? 2 : 0;
        // two stages
        const LtProbe0 p = lt_probe0(lt, key);
        const uint32_t *t0 = lt.tags + 2u * p.b0, *t1 = lt.tags + 2u * p.b1;
        const LtExact x = lt_exact_stage(p, U2{t0[0], t0[1]}, U2{t1[0], t1[1]}, cand, forced);
        int got = x.hit ? 1 : 0;
        uint32_t slot = x.slot;
        out[2] += x.batch;
        if (NEAR && x.batch) {
            const uint32_t lo = (uint32_t)key, hi = lt_rec_hi(key, forced);
            const LtVerdict v = decide<NEAR>(lt, lt_rec_key(lo, hi), lt_rec_forced(hi));
            got = v.perfect ? 1 : v.imperfect ? 2 : 0;
            slot = v.slot;
        }
        if (got == 1) out[0]++;
        if (got == 2) out[1]++;
        if (got != ref || (got != 0 && slot != r.slot)) out[3]++;
    }
}
}

extern "C" {

// the 2-bit key of each feature (f2q_host.h: feature_key), 2L bits, base i at bits 2i..2i+1; ~0 if it has none
void lts_feature_keys(const char *seqs, const uint32_t *offs, uint32_t n, uint64_t *keys)
{
    for (uint32_t f = 0; f < n; f++) {
        uint64_t k;
        keys[f] = feature_key((const uint8_t *)seqs + offs[f], offs[f + 1] - offs[f], k) ? k : ~0ull;
    }
}

// Builds the LDS tables of the library (n features of length L, concatenated, offsets offs[0..n]) and decides n_reads
// keys both ways.  out[0..3]: perfect, imperfect, batch candidates, reads where the two disagree (verdict or slot).
// Returns -1 when the library gets no LDS tables.
int lts_check(const char *seqs, const uint32_t *offs, uint32_t n, int L, int near, const uint64_t *keys, const uint32_t *forced,
              const uint8_t *cand, uint32_t n_reads, uint64_t *out)
{
    HostIndex ix;
    build_index(ix, seqs, offs, n, near ? 1 : 0, L);
    if (!ix.lt.ok) return -1;
    LtDesc lt = ix.lt;
    lt.tags = ix.lt_tags.data(); lt.slot_of = ix.lt_slot_of.data(); lt.feat_of = ix.lt_feat_of.data();
    memset(out, 0, 4 * sizeof(uint64_t));
    if (near) run<true>(lt, keys, forced, cand, n_reads, out);
    else run<false>(lt, keys, forced, cand, n_reads, out);
    return 0;
}

// One tile of the batch stage's compaction as the kernel does it, ds_permute simulated: a sender writes its value to
// lane addr / 4, and when several write one lane the outcome is taken as unknown.  batch[lane * 4 + j] != 0 marks the
// candidates.  Returns the number of candidates, or -1 when one is lost, duplicated, or a receiving lane takes a value
// that is unknown or not its candidate's.
int lts_compact(const uint8_t *batch)
{
    uint32_t pre[5] = {0, 0, 0, 0, 0}, pos[64][4];
    for (int j = 0; j < 4; j++) {
        uint32_t c = 0;
        for (int l = 0; l < 64; l++) { pos[l][j] = pre[j] + c; c += batch[l * 4 + j] != 0; }
        pre[j + 1] = pre[j] + c;
    }
    std::vector<int> seen(256, 0);
    for (uint32_t lo = 0; lo < pre[4]; lo += 64u) {
        uint32_t got[64];
        bool have[64] = {};
        for (int j = 0; j < 4; j++) {
            if (!lt_batch_has(pre, j, lo)) continue;
            int writers[64] = {};
            uint32_t val[64] = {};
            for (int l = 0; l < 64; l++) {                       // every lane of the wave is active and writes
                const bool send = batch[l * 4 + j] && pos[l][j] - lo < 64u;
                const uint32_t to = (send ? pos[l][j] - lo : lt_dump(pre, j, lo)) % 64u;
                writers[to]++;
                val[to] = send ? (uint32_t)(l * 4 + j) : 0xFFFFu;   // a non-sender's value is garbage
            }
            for (uint32_t t = 0; t < 64; t++) {
                const uint32_t at = lo + t;
                if (!(at >= pre[j] && at < pre[j + 1])) continue;
                if (writers[t] != 1 || val[t] == 0xFFFFu || have[t]) return -1;
                got[t] = val[t]; have[t] = true;
            }
        }
        for (uint32_t t = 0; t < 64; t++) {
            const bool valid = lo + t < pre[4];
            if (valid != have[t]) return -1;
            if (valid) {
                if (seen[got[t]]++ || !batch[got[t]] || pos[got[t] / 4][got[t] % 4] != lo + t) return -1;
            }
        }
    }
    for (int i = 0; i < 256; i++)
        if ((batch[i] != 0) != (seen[i] == 1)) return -1;
    return (int)pre[4];
}

}
