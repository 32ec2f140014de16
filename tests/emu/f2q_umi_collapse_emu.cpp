// tests/emu/f2q_umi_collapse_emu.cpp -- TEST INFRASTRUCTURE.  The per-lane logic of f2q_umi_collapse (umi_find, uf_find /
// uf_union, umi_link_one, umi_root_one of 2fast2q_amd/csrc/f2q_device.h) compiled with g++ and run over the emulated
// (feature, UMI) set of f2q_umi_emu.cpp (included whole): parent[i] = i, every neighbour of every occupied slot, the
// roots -- what k_umi_uf_init, k_umi_link and k_umi_roots do, one lane at a time.  The product never uses this file.
// -DF2Q_UMI_COLLAPSE_EMU_MAIN: a stand-alone program over known answers (for -fsanitize=address,undefined builds).
#include "f2q_umi_emu.cpp"

extern "C" {

// molecules[n_features], extra[2] = pairs held, edges; order 0: the slots front to back, 1: back to front (the result
// does not depend on it).  0, or -1 for a dist other than 0 / 1
int uemu_collapse(void *h, int32_t dist, int32_t order, int64_t *molecules, int64_t *extra)
{
    UEmu *x = (UEmu *)h;
    const uint32_t nf = x->e->ix.n_features;
    if (dist != 0 && dist != 1) return -1;
    extra[0] = (int64_t)x->ctr[F2Q_UMI_HELD]; extra[1] = 0;
    if (dist == 0 || x->slots.empty()) {
        for (uint32_t f = 0; f < nf; f++) molecules[f] = x->slots.empty() ? 0 : (int64_t)x->umis[f];
        return 0;
    }
    const uint32_t slots = (uint32_t)x->slots.size(), per = 3u * (uint32_t)x->u.length;
    std::vector<uint32_t> parent(slots);
    for (uint32_t i = 0; i < slots; i++) parent[i] = i;
    std::vector<unsigned long long> mol(std::max<uint32_t>(nf, 1), 0ull);
    for (uint32_t a = 0; a < slots; a++) {
        const uint32_t i = order ? slots - 1 - a : a;
        const unsigned long long k = x->slots[i];
        if (k == KEY_EMPTY) continue;
        for (uint32_t n = 0; n < per; n++) extra[1] += umi_link_one(x->u, parent.data(), i, k, n);
    }
    for (uint32_t i = 0; i < slots; i++) {
        if (parent[i] > i) return -2;                                // the forest's invariant
        umi_root_one(x->u, parent.data(), mol.data(), i);
    }
    for (uint32_t f = 0; f < nf; f++) molecules[f] = (int64_t)mol[f];
    return 0;
}

}

#ifdef F2Q_UMI_COLLAPSE_EMU_MAIN
static std::string umi_text(uint32_t code, int len)
{
    std::string s;
    for (int j = 0; j < len; j++) s += "ACGT"[(code >> (2 * j)) & 3u];
    return s;
}

// the known answers of four bases (all 256 UMIs on one feature; two near and one far; the same UMI on two adjacent
// features) from a set of 64 slots that grows, then a chain of sixteen-base UMIs with a substitution in the top field
int main()
{
    uint64_t z = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { z ^= z << 13; z ^= z >> 7; z ^= z << 17; return z; };
    const int NG = 12, GL = 20;
    std::string seqs; std::vector<uint32_t> offs(1, 0);
    for (int g = 0; g < NG; g++) { for (int j = 0; j < GL; j++) seqs += "ACGT"[rnd() & 3]; offs.push_back((uint32_t)seqs.size()); }
    f2q_params p; memset(&p, 0, sizeof p);
    p.mode = 0; p.miss = 0; p.phred = 30; p.length = GL; p.n_start = 1; p.start[0] = 0; p.qual_up = p.qual_down = 30;
    auto fastq = [&](const std::vector<std::pair<int, std::string>> &reads) {
        std::string fq;
        for (auto &r : reads) { const std::string s = seqs.substr((size_t)r.first * GL, GL) + r.second + "ACGTACGTAC"; fq += "@r\n" + s + "\n+\n" + std::string(s.size(), 'I') + "\n"; }
        return fq;
    };
    bool ok = true;
    {
        void *h = uemu_create(&p, GL, 4, 64);
        if (!h) return 2;
        uemu_set_features(h, seqs.data(), offs.data(), NG);
        std::vector<int64_t> mol(NG, -1); int64_t extra[2];
        if (uemu_collapse(h, 1, 0, mol.data(), extra) != 0) return 3;             // nothing counted yet
        for (int64_t v : mol) ok = ok && v == 0;
        ok = ok && extra[0] == 0 && extra[1] == 0;
        std::vector<std::pair<int, std::string>> reads;
        for (uint32_t c = 0; c < 256; c++) reads.push_back({0, umi_text(c, 4)});
        for (const char *u : {"AAAA", "AAAC", "GGGG", "AAAA"}) reads.push_back({1, u});
        for (const char *u : {"ACGT", "ACGA"}) reads.push_back({2, u});
        reads.push_back({3, "ACGT"});
        for (size_t at = 0; at < reads.size(); at += 40) {
            const std::string fq = fastq(std::vector<std::pair<int, std::string>>(reads.begin() + at, reads.begin() + std::min(at + 40, reads.size())));
            if (uemu_count_block(h, (const uint8_t *)fq.data(), fq.size()) != fq.size()) return 4;
        }
        for (int order = 0; order < 2; order++) {
            if (uemu_collapse(h, 1, order, mol.data(), extra) != 0) return 5;
            const int64_t want[4] = {1, 2, 1, 1};
            for (int g = 0; g < NG; g++) ok = ok && mol[g] == (g < 4 ? want[g] : 0);
            ok = ok && extra[0] == 262 && extra[1] == 1538;
            printf("L=4 order %d: molecules %lld %lld %lld %lld, pairs %lld, edges %lld\n", order, (long long)mol[0], (long long)mol[1],
                   (long long)mol[2], (long long)mol[3], (long long)extra[0], (long long)extra[1]);
        }
        std::vector<int64_t> counts(NG), umis(NG); int64_t stats[5], ue[2];
        uemu_read(h, counts.data(), stats, umis.data(), ue);
        if (uemu_collapse(h, 0, 0, mol.data(), extra) != 0) return 6;
        ok = ok && mol == umis && extra[1] == 0 && uemu_collapse(h, 2, 0, mol.data(), extra) == -1;
        uemu_destroy(h);
    }
    {
        void *h = uemu_create(&p, GL, 16, 64);
        if (!h) return 7;
        uemu_set_features(h, seqs.data(), offs.data(), NG);
        std::vector<std::pair<int, std::string>> reads;
        std::string u(16, 'T');
        for (int step = 0; step < 10; step++) {                      // a chain: each UMI one base from the one before
            reads.push_back({5, u});
            const int at = step == 0 ? 15 : (int)(rnd() % 16);       // (the first step changes the top field)
            u[at] = u[at] == 'A' ? 'C' : 'A';
        }
        reads.push_back({5, std::string(16, 'G')});                  // far from all of them
        reads.push_back({6, std::string(16, 'T')});                  // the chain's first UMI on the next feature
        const std::string fq = fastq(reads);
        if (uemu_count_block(h, (const uint8_t *)fq.data(), fq.size()) != fq.size()) return 8;
        std::vector<int64_t> mol(NG), umis(NG), counts(NG); int64_t extra[2], stats[5], ue[2];
        uemu_read(h, counts.data(), stats, umis.data(), ue);
        if (uemu_collapse(h, 1, 0, mol.data(), extra) != 0) return 9;
        printf("L=16 chain: umis %lld, molecules %lld and %lld, pairs %lld, edges %lld\n", (long long)umis[5], (long long)mol[5], (long long)mol[6],
               (long long)extra[0], (long long)extra[1]);
        ok = ok && mol[5] == 2 && mol[6] == 1 && extra[0] == umis[5] + 1 && extra[1] >= umis[5] - 2;
        uemu_destroy(h);
    }
    return ok ? 0 : 1;
}
#endif
