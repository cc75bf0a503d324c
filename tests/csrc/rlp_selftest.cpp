// Stand-alone run of the RLP harness (rlp_harness.cpp) for a sanitizer build
// (make rlp_selftest: g++ -fsanitize=address,undefined): the round trips and the
// refused inputs of tests/test_rlp_cpu.py.  rlp_decode_bi hands the reader a
// heap copy of exactly the input's length, so a read outside the input is a
// heap-buffer-overflow report.  Exit status 0: every case as expected.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

extern "C" {
uint64_t rlp_encode_bi(uint32_t B, const uint32_t *last, const uint32_t *creator, uint32_t V, const uint32_t *by_off,
                       const uint32_t *by, uint8_t *out, uint64_t cap);
int rlp_decode_bi(const uint8_t *in, uint32_t n, uint32_t cap_b, uint32_t *last, uint32_t *creator, uint32_t cap_v,
                  uint32_t *by_off, uint32_t cap_by, uint32_t *by, uint32_t counts[4]);
}

namespace {

using Bytes = std::vector<uint8_t>;
struct Tables {
    std::vector<uint32_t> last, creator;
    std::vector<std::vector<uint32_t>> by;
};
int failures = 0;

void check(bool ok, const char *what, size_t k = 0) {
    if (!ok) {
        fprintf(stderr, "FAILED: %s (%zu)\n", what, k);
        failures++;
    }
}

Bytes encode(const Tables &t) {
    std::vector<uint32_t> off{0}, flat;
    for (const auto &l : t.by) {
        flat.insert(flat.end(), l.begin(), l.end());
        off.push_back((uint32_t)flat.size());
    }
    const uint32_t B = (uint32_t)t.last.size(), V = (uint32_t)t.by.size();
    Bytes out(rlp_encode_bi(B, t.last.data(), t.creator.data(), V, off.data(), flat.data(), nullptr, 0));
    rlp_encode_bi(B, t.last.data(), t.creator.data(), V, off.data(), flat.data(), out.data(), out.size());
    return out;
}

bool decode(const Bytes &in, Tables *t) {
    const uint32_t cap = 4096;
    std::vector<uint32_t> last(cap), cr(cap), off(cap + 1), by(cap);
    uint32_t c[4] = {0, 0, 0, 0};
    if (rlp_decode_bi(in.data(), (uint32_t)in.size(), cap, last.data(), cr.data(), cap, off.data(), cap, by.data(), c) != 1)
        return false;
    t->last.assign(last.begin(), last.begin() + c[0]);
    t->creator.assign(cr.begin(), cr.begin() + c[1]);
    t->by.clear();
    for (uint32_t v = 0; v < c[2]; v++) t->by.emplace_back(by.begin() + off[v], by.begin() + off[v + 1]);
    return true;
}

Tables singles(std::vector<uint32_t> last) {
    Tables t;
    t.last = std::move(last);
    for (uint32_t i = 0; i < t.last.size(); i++) {
        t.creator.push_back(i);
        t.by.push_back({i});
    }
    return t;
}

Bytes with(Bytes b, size_t at, uint8_t v) {
    b[at] = v;
    return b;
}

Bytes cat(Bytes a, const Bytes &b, size_t from = 0) {
    a.insert(a.end(), b.begin() + from, b.end());
    return a;
}

}  // namespace

int main() {
    const Bytes example = {0xce, 0xc3, 0x03, 0x80, 0x02, 0xc3, 0x80, 0x01, 0x80, 0xc5, 0xc2, 0x80, 0x02, 0xc1, 0x01};
    const std::vector<uint32_t> uints = {0, 0x7F, 0x80, 0xFF, 0x100, 0xFFFFFF, 0x1000000, 0xFFFFFFFFu};
    std::vector<Tables> cases = {singles(uints), singles(std::vector<uint32_t>(55, 1)), singles(std::vector<uint32_t>(56, 1)),
                                 singles(std::vector<uint32_t>(60, 200)),
                                 Tables{{3, 5, 2, 7, 9}, {0, 1, 2, 1, 1}, {{0}, {1, 3, 4}, {2}}},
                                 Tables{{3, 0, 2}, {0, 1, 0}, {{0, 2}, {1}}}, Tables{}};
    Tables u = singles(std::vector<uint32_t>(8, 1));
    u.creator = uints;
    for (size_t i = 0; i < 8; i++) u.by[i] = {uints[i]};
    cases.push_back(u);
    for (size_t k = 0; k < cases.size(); k++) {
        Tables back;
        const Bytes e = encode(cases[k]);
        check(decode(e, &back), "decodes", k);
        check(back.last == cases[k].last && back.creator == cases[k].creator && back.by == cases[k].by, "round trip", k);
    }
    check(encode(cases[5]) == example, "the example's bytes");
    check(encode(cases[3])[0] == 0xF9, "60 branches: 0xF9 header");

    Tables t;
    std::vector<Bytes> refused = {{}, cat(example, {0x00}), with(example, 0, 0x80 + 14), with(example, 1, 0x83),
                                  with(example, 10, 0x82)};
    for (size_t k = 1; k < example.size(); k++) refused.emplace_back(example.begin(), example.begin() + k);
    refused.push_back({0xcc, 0xc6, 0x85, 0x01, 0x00, 0x00, 0x00, 0x00, 0xc1, 0x80, 0xc2, 0xc1, 0x80});   // a 5-byte uint
    refused.push_back(with(with(with(example, 2, 0xb9), 3, 0xff), 4, 0xff));   // long string, length past the end
    refused.push_back(cat({0xf9, 0xff, 0xff}, example, 1));                    // long list, length past the end
    refused.push_back({0xfb, 0x00, 0x00});                                     // its length bytes past the end
    const Bytes ff8 = {0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff};
    refused.push_back(cat(ff8, example, 1));                                   // hl + len wraps: outer list
    refused.push_back(cat(cat({0xc0 + 9 + 14}, ff8), example, 1));             // ... and an inner one
    // two inner headers whose hl + len wraps to 8, then an empty long-form list: a reader that adds
    // before it compares accepts this as three empty lists
    Bytes wrapped = {0xd9};
    wrapped.insert(wrapped.end(), 17, 0xff);
    wrapped.insert(wrapped.end(), 8, 0x00);
    refused.push_back(wrapped);
    for (size_t k = 0; k < refused.size(); k++) check(!decode(refused[k], &t), "refused", k);

    printf("rlp selftest: %zu round trips, %zu refused inputs, %d failures\n", cases.size(), refused.size(), failures);
    return failures ? 1 : 0;
}
