// lx_rlp.h -- go-ethereum rlp (v1.9.22) of BranchesInfo{[]idx.Event,
// []idx.Validator, [][]idx.Validator} (vecengine/branches_info.go:9-13), as
// write-back emits it and the load reads it back (lx_index_persist.cpp):
// structs and slices are lists, uints are minimal big-endian strings (0 = 0x80,
// < 0x80 = the byte).  The reader is the one part of the host engine that
// parses bytes a caller supplies; no HIP here, so that it is tested on the CPU
// (tests/csrc/rlp_harness.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#pragma GCC visibility push(hidden)   // internal to the library that includes it
namespace lxi {

inline void rlp_uint(std::string &o, uint32_t x) {
    if (x == 0) { o.push_back((char)0x80); return; }
    if (x < 0x80) { o.push_back((char)x); return; }
    const int nb = (x >> 24) ? 4 : (x >> 16) ? 3 : (x >> 8) ? 2 : 1;
    o.push_back((char)(0x80 + nb));
    for (int i = nb - 1; i >= 0; i--) o.push_back((char)(x >> (8 * i)));
}

inline void rlp_list(std::string &o, const std::string &payload) {
    const uint64_t n = payload.size();
    if (n <= 55) {
        o.push_back((char)(0xC0 + n));
    } else {
        int nb = 0;
        for (uint64_t t = n; t; t >>= 8) nb++;
        o.push_back((char)(0xF7 + nb));
        for (int i = nb - 1; i >= 0; i--) o.push_back((char)(n >> (8 * i)));
    }
    o += payload;
}

// BranchIDLastSeq, BranchIDCreatorIdxs (per branch), BranchIDByCreators (per creator)
inline std::string encode_branches_info(const std::vector<uint32_t> &last_seq, const std::vector<uint32_t> &creator,
                                        const std::vector<std::vector<uint32_t>> &by_creator) {
    std::string last, cr, by, body, out;
    for (uint32_t s : last_seq) rlp_uint(last, s);
    for (uint32_t c : creator) rlp_uint(cr, c);
    for (const auto &l : by_creator) {
        std::string x;
        for (uint32_t b : l) rlp_uint(x, b);
        rlp_list(by, x);
    }
    rlp_list(body, last);
    rlp_list(body, cr);
    rlp_list(body, by);
    rlp_list(out, body);
    return out;
}

// reader: a list of three lists (uint, uint, list of uint lists)
struct RlpIn {
    const uint8_t *p, *end;
    bool ok = true;
    // header of the next item: list?, payload bounds (inside [p, end))
    bool item(bool *list, const uint8_t **b, const uint8_t **e) {
        if (p >= end) return ok = false;
        const uint8_t x = *p;
        uint64_t len = 0, hl = 1;
        if (x < 0x80) { *list = false; *b = p; *e = p + 1; p++; return true; }
        if (x <= 0xB7) { *list = false; len = x - 0x80; }
        else if (x <= 0xBF) { *list = false; hl += x - 0xB7; }
        else if (x <= 0xF7) { *list = true; len = x - 0xC0; }
        else { *list = true; hl += x - 0xF7; }
        const uint64_t left = (uint64_t)(end - p);
        if (hl > 1) {
            if (left < hl || hl > 9) return ok = false;
            for (uint64_t k = 1; k < hl; k++) len = (len << 8) | p[k];
        }
        if (len > left - hl) return ok = false;   // (hl + len would wrap for a length near 2^64)
        *b = p + hl;
        *e = p + hl + len;
        p = *e;
        return true;
    }
    bool uint_list(const uint8_t *b, const uint8_t *e, std::vector<uint32_t> &out) {
        RlpIn r{b, e};
        while (r.p < r.end) {
            bool l;
            const uint8_t *x, *y;
            if (!r.item(&l, &x, &y) || l || y - x > 4) return ok = false;
            uint32_t v = 0;
            for (const uint8_t *q = x; q < y; q++) v = (v << 8) | *q;
            out.push_back(v);
        }
        return true;
    }
};

inline bool decode_branches_info(const uint8_t *d, uint32_t n, std::vector<uint32_t> &last, std::vector<uint32_t> &cr,
                                 std::vector<std::vector<uint32_t>> &by) {
    RlpIn r{d, d + n};
    bool l;
    const uint8_t *b, *e;
    if (!r.item(&l, &b, &e) || !l || r.p != r.end) return false;
    RlpIn body{b, e};
    const uint8_t *x, *y;
    if (!body.item(&l, &x, &y) || !l || !body.uint_list(x, y, last)) return false;
    if (!body.item(&l, &x, &y) || !l || !body.uint_list(x, y, cr)) return false;
    if (!body.item(&l, &x, &y) || !l) return false;
    RlpIn lists{x, y};
    while (lists.p < lists.end) {
        const uint8_t *u, *v;
        if (!lists.item(&l, &u, &v) || !l) return false;
        by.emplace_back();
        if (!lists.uint_list(u, v, by.back())) return false;
    }
    return body.p == body.end && body.ok && lists.ok;
}

}  // namespace lxi
#pragma GCC visibility pop
