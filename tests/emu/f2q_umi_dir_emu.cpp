// tests/emu/f2q_umi_dir_emu.cpp -- TEST INFRASTRUCTURE.  The per-lane logic of f2q_umi_collapse_directional
// (umi_link_dir_one, umi_dir_spread_one, umi_dir_root_one of 2fast2q_amd/csrc/f2q_device.h) compiled with g++ and run over
// the emulated set of f2q_umi_emu.cpp with reads kept (included through f2q_umi_collapse_emu.cpp, whose cluster pass
// serves the comparisons): what k_umi_link<true>, k_umi_dir_spread and k_umi_dir_roots do, one lane at a time.  The
// product never uses this file.
// -DF2Q_UMI_DIR_EMU_MAIN: a stand-alone program over known answers (for -fsanitize=address,undefined builds).
#include "f2q_umi_collapse_emu.cpp"

extern "C" {

// uemu_create with reads kept per pair (f2q_set_umi_reads); every uemu_* call takes the handle
void *demu_create(const f2q_params *p, int32_t start, int32_t length, uint64_t min_slots)
{
    UEmu *x = (UEmu *)uemu_create(p, start, length, min_slots);
    if (x) x->keep_reads = true;
    return x;
}

// molecules[n_features], extra[4] = pairs held, unordered Hamming-1 pairs, slots the link flagged, sum of reads.  order
// 0: the slots front to back, 1: back to front, >= 2: shuffled with `order` as the seed, in the link and in the spread
// (the result does not depend on it).  0, or -2 when the forest's invariant is broken
int demu_directional(void *h, int32_t order, int64_t *molecules, int64_t *extra)
{
    UEmu *x = (UEmu *)h;
    const uint32_t nf = x->e->ix.n_features;
    for (uint32_t f = 0; f < nf; f++) molecules[f] = 0;
    extra[0] = (int64_t)x->ctr[F2Q_UMI_HELD]; extra[1] = extra[2] = extra[3] = 0;
    if (x->slots.empty()) return 0;
    const uint32_t slots = (uint32_t)x->slots.size(), per = 3u * (uint32_t)x->u.length;
    std::vector<uint32_t> parent(slots), dom(slots, 0u), visit(slots);
    for (uint32_t i = 0; i < slots; i++) { parent[i] = i; visit[i] = order == 1 ? slots - 1 - i : i; }
    if (order >= 2) {
        uint64_t z = 0x9E3779B97F4A7C15ull * (uint64_t)order;
        for (uint32_t i = slots - 1; i > 0; i--) { z ^= z << 13; z ^= z >> 7; z ^= z << 17; std::swap(visit[i], visit[z % (i + 1)]); }
    }
    std::vector<unsigned long long> mol(std::max<uint32_t>(nf, 1), 0ull);
    for (uint32_t i : visit) {
        const unsigned long long k = x->slots[i];
        if (k == KEY_EMPTY) continue;
        for (uint32_t n = 0; n < per; n++) extra[1] += umi_link_dir_one(x->u, parent.data(), dom.data(), i, k, x->reads[i], n);
    }
    for (uint32_t i = 0; i < slots; i++) if (parent[i] > i) return -2;
    for (uint32_t i : visit) umi_dir_spread_one(x->u, parent.data(), dom.data(), i);
    unsigned long long tot[2] = {0, 0};
    for (uint32_t i = 0; i < slots; i++) umi_dir_root_one(x->u, parent.data(), dom.data(), mol.data(), i, tot);
    extra[2] = (int64_t)tot[0]; extra[3] = (int64_t)tot[1];
    for (uint32_t f = 0; f < nf; f++) molecules[f] = (int64_t)mol[f];
    return 0;
}

// the pairs with their reads sorted by (feature, codes), and the slot each sits in; returns how many (arrays may be null)
uint64_t demu_pairs(void *h, uint64_t cap, uint32_t *feature, uint32_t *codes, uint32_t *reads, uint32_t *slot)
{
    UEmu *x = (UEmu *)h;
    std::vector<std::pair<unsigned long long, uint32_t>> held;
    for (uint32_t i = 0; i < (uint32_t)x->slots.size(); i++) if (x->slots[i] != KEY_EMPTY) held.emplace_back(x->slots[i], i);
    std::sort(held.begin(), held.end());
    if (feature) for (size_t i = 0; i < held.size() && i < cap; i++) {
        feature[i] = (uint32_t)(held[i].first >> 32); codes[i] = (uint32_t)held[i].first;
        reads[i] = x->reads[held[i].second]; slot[i] = held[i].second;
    }
    return held.size();
}

}

#ifdef F2Q_UMI_DIR_EMU_MAIN
// one feature per case, UMI 20,4, from a set of 8 slots that grows: 10/1/1 on a chain, 3/3, 2/2, 2/1, 3/2, a chain of
// three single reads, two single reads next to five
int main()
{
    uint64_t z = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { z ^= z << 13; z ^= z >> 7; z ^= z << 17; return z; };
    const int NG = 12, GL = 20;
    std::string seqs; std::vector<uint32_t> offs(1, 0);
    for (int g = 0; g < NG; g++) { for (int j = 0; j < GL; j++) seqs += "ACGT"[rnd() & 3]; offs.push_back((uint32_t)seqs.size()); }
    f2q_params p; memset(&p, 0, sizeof p);
    p.mode = 0; p.miss = 0; p.phred = 30; p.length = GL; p.n_start = 1; p.start[0] = 0; p.qual_up = p.qual_down = 30;
    struct Case { int f; const char *u; int c; };
    const Case cases[] = {{0, "AAAA", 10}, {0, "AAAC", 1}, {0, "AACC", 1}, {1, "AAAA", 3}, {1, "AAAC", 3}, {2, "AAAA", 2}, {2, "AAAC", 2},
                          {3, "AAAA", 2}, {3, "AAAC", 1}, {4, "AAAA", 3}, {4, "AAAC", 2}, {5, "AAAA", 1}, {5, "AAAC", 1}, {5, "AACC", 1},
                          {6, "AAAA", 1}, {6, "AAAC", 1}, {6, "AACC", 5}};
    const int64_t want[NG] = {1, 2, 2, 1, 1, 1, 1, 0, 0, 0, 0, 0}, want_cluster[NG] = {1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
    std::vector<std::pair<int, std::string>> reads;
    int total = 0;
    for (const Case &c : cases) for (int i = 0; i < c.c; i++) { reads.push_back({c.f, c.u}); total++; }
    for (size_t i = reads.size() - 1; i > 0; i--) std::swap(reads[i], reads[rnd() % (i + 1)]);
    void *h = demu_create(&p, GL, 4, 8);
    if (!h) return 2;
    uemu_set_features(h, seqs.data(), offs.data(), NG);
    std::vector<int64_t> mol(NG, -1), cl(NG, -1); int64_t extra[4], ce[2];
    if (demu_directional(h, 0, mol.data(), extra) != 0) return 3;                 // nothing counted yet
    bool ok = extra[0] == 0 && extra[1] == 0 && extra[2] == 0 && extra[3] == 0;
    for (int64_t v : mol) ok = ok && v == 0;
    for (size_t at = 0; at < reads.size(); at += 5) {
        std::string fq;
        for (size_t i = at; i < std::min(at + 5, reads.size()); i++) {
            const std::string s = seqs.substr((size_t)reads[i].first * GL, GL) + reads[i].second + "ACGTACGTAC";
            fq += "@r\n" + s + "\n+\n" + std::string(s.size(), 'I') + "\n";
        }
        if (uemu_count_block(h, (const uint8_t *)fq.data(), fq.size()) != fq.size()) return 4;
    }
    for (int order = 0; order < 4; order++) {
        if (demu_directional(h, order, mol.data(), extra) != 0) return 5;
        if (uemu_collapse(h, 1, 0, cl.data(), ce) != 0) return 6;
        for (int g = 0; g < NG; g++) ok = ok && mol[g] == want[g] && cl[g] == want_cluster[g];
        ok = ok && extra[0] == 17 && extra[1] == ce[1] && extra[2] == 4 && extra[3] == total && ce[0] == 17;
        printf("order %d: molecules %lld %lld %lld %lld %lld %lld %lld, pairs %lld, edges %lld, dominated %lld, reads %lld, rehashes %llu\n", order,
               (long long)mol[0], (long long)mol[1], (long long)mol[2], (long long)mol[3], (long long)mol[4], (long long)mol[5], (long long)mol[6],
               (long long)extra[0], (long long)extra[1], (long long)extra[2], (long long)extra[3], (unsigned long long)((UEmu *)h)->rehashes);
    }
    ok = ok && ((UEmu *)h)->rehashes >= 1;
    std::vector<uint32_t> f(17), c(17), r(17), s(17);
    ok = ok && demu_pairs(h, 17, f.data(), c.data(), r.data(), s.data()) == 17 && f[0] == 0 && c[0] == 0 && r[0] == 10;
    uemu_reset(h);
    if (demu_directional(h, 0, mol.data(), extra) != 0) return 7;
    ok = ok && extra[0] == 0 && extra[3] == 0;
    uemu_destroy(h);
    return ok ? 0 : 1;
}
#endif
