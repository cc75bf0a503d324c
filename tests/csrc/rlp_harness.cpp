// C entry points over the BranchesInfo RLP writer and reader (csrc/lx_rlp.h)
// for tests/test_rlp_cpu.py.  The tables travel flat: per branch last seq and
// creator, then the branches of every creator one list after the other
// (by_off[c] .. by_off[c + 1]).
#include <cstring>

#include "lx_rlp.h"

extern "C" {

// the encoding's length; its bytes into out when cap holds them
uint64_t rlp_encode_bi(uint32_t B, const uint32_t *last, const uint32_t *creator, uint32_t V, const uint32_t *by_off,
                       const uint32_t *by, uint8_t *out, uint64_t cap) {
    std::vector<std::vector<uint32_t>> lists(V);
    for (uint32_t c = 0; c < V; c++) lists[c].assign(by + by_off[c], by + by_off[c + 1]);
    const std::string s = lxi::encode_branches_info(std::vector<uint32_t>(last, last + B),
                                                    std::vector<uint32_t>(creator, creator + B), lists);
    if (out && s.size() <= cap) memcpy(out, s.data(), s.size());
    return s.size();
}

// 1 and the tables when `in` is a well-formed BranchesInfo, else 0.  The input
// is copied into a block of exactly n bytes first, so that a read outside it
// is one outside an allocation (the sanitizer build of rlp_selftest sees it).
// counts: {B of last, B of creator, V, entries of by}; -1 when a table does not
// fit its capacity.
int rlp_decode_bi(const uint8_t *in, uint32_t n, uint32_t cap_b, uint32_t *last, uint32_t *creator, uint32_t cap_v,
                  uint32_t *by_off, uint32_t cap_by, uint32_t *by, uint32_t counts[4]) {
    uint8_t *exact = new uint8_t[n ? n : 1];
    if (n) memcpy(exact, in, n);
    std::vector<uint32_t> l, c;
    std::vector<std::vector<uint32_t>> lists;
    const bool ok = lxi::decode_branches_info(n ? exact : nullptr, n, l, c, lists);
    delete[] exact;
    if (!ok) return 0;
    uint64_t nby = 0;
    for (const auto &x : lists) nby += x.size();
    counts[0] = (uint32_t)l.size();
    counts[1] = (uint32_t)c.size();
    counts[2] = (uint32_t)lists.size();
    counts[3] = (uint32_t)nby;
    if (l.size() > cap_b || c.size() > cap_b || lists.size() > cap_v || nby > cap_by) return -1;
    if (!l.empty()) memcpy(last, l.data(), l.size() * 4);
    if (!c.empty()) memcpy(creator, c.data(), c.size() * 4);
    uint32_t o = 0;
    for (size_t v = 0; v < lists.size(); v++) {
        by_off[v] = o;
        for (uint32_t b : lists[v]) by[o++] = b;
    }
    by_off[lists.size()] = o;
    return 1;
}

}  // extern "C"
