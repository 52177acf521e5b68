// tests/reveal_statement_check.cpp -- the mask-slice rule of selective disclosure on both of its sides, stand-alone, host only (built under ASan + UBSan by
// tests/test_reveal_host.py with circuit.cpp, marlin_codec.cpp and capi_host.cpp; nothing is loaded into python).  The prover reaches the rule as zk::chunk_mask_slice
// and zk::reveal_bytes (csrc/statement.hpp), a verifier as the tail of row j of zkaes_chunk_public_inputs_rv: row j must be row j of zkaes_chunk_public_inputs, then the
// bits of mask bytes [chunk j / 8, chunk (j + 1) / 8), then the bits of revealed[chunk j, chunk (j + 1)) -- for ECB, CBC and CTR, slices of 16 and 32 bytes, 1, 2 and 3
// chunks, with and without a key tag and states, in heap buffers of exactly their size -- and zkaes_reveal_bytes must be zk::reveal_bytes.  The two invalid arguments
// (a mask bit at or beyond the length, a non-zero revealed byte under a zero mask bit) are errors of every entry that takes them.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>
#include "statement.hpp"
#include "../include/zkaes.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

static std::vector<uint8_t> bits_of(const uint8_t *bytes, size_t n) {
    std::vector<uint8_t> out;
    for (size_t i = 0; i < n; i++) for (int b = 0; b < 8; b++) out.push_back((bytes[i] >> b) & 1);
    return out;
}
static std::vector<uint8_t> stream(size_t n, uint32_t seed) {
    std::vector<uint8_t> out(n);
    for (size_t i = 0; i < n; i++) { seed = seed * 1664525u + 1013904223u; out[i] = (uint8_t)(seed >> 24); }
    return out;
}
static std::unique_ptr<uint8_t[]> exact(const std::vector<uint8_t> &v) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[v.size() ? v.size() : 1]);
    if (!v.empty()) memcpy(p.get(), v.data(), v.size());
    return p;
}

int main() {
    const int kinds[3] = {ZKAES_CIRCUIT_AES, ZKAES_CIRCUIT_AES_CBC, ZKAES_CIRCUIT_AES_CTR};
    size_t cases = 0;
    for (int kind : kinds) for (size_t chunk : {(size_t)16, (size_t)32}) for (size_t n : {(size_t)1, (size_t)2, (size_t)3}) for (size_t tag_len : {(size_t)0, (size_t)32}) for (int with_states = 0; with_states < 2; with_states++) {
        const uint32_t seed = (uint32_t)(kind * 1000 + chunk * 100 + n * 10 + tag_len + with_states);
        const size_t len = chunk * n;
        const std::vector<uint8_t> ct = stream(len, seed), msg = stream(len, seed + 4), tag = stream(32, seed + 1), states = stream(32 * (n + 1), seed + 2), hdr0 = stream(16, seed + 3), mask = stream(len / 8, seed + 5);
        std::vector<uint8_t> revealed(len), by_abi(len);
        zk::reveal_bytes(msg.data(), mask.data(), len, revealed.data());
        auto m = exact(mask), r = exact(revealed), c = exact(ct), mm = exact(msg);
        CHECK(zkaes_reveal_bytes(mm.get(), len, m.get(), len / 8, by_abi.data()) == 0 && by_abi == revealed, "zkaes_reveal_bytes");
        for (size_t i = 0; i < len; i++) CHECK(revealed[i] == (((mask[i / 8] >> (i % 8)) & 1) ? msg[i] : 0), "byte %zu", i);
        const uint8_t *h0 = kind == ZKAES_CIRCUIT_AES ? nullptr : hdr0.data(), *tg = tag_len ? tag.data() : nullptr, *st = with_states ? states.data() : nullptr;
        size_t bits = 0, bits_rv = 0;
        CHECK(zkaes_chunk_public_inputs(kind, n, h0, c.get(), len, tg, tag_len, st, nullptr, &bits) == 0, "%s", zkaes_last_error());
        CHECK(zkaes_chunk_public_inputs_rv(kind, n, h0, c.get(), len, tg, tag_len, st, m.get(), len / 8, r.get(), nullptr, &bits_rv) == 0, "%s", zkaes_last_error());
        CHECK(bits_rv == bits + chunk + 8 * chunk, "row length");
        std::vector<uint8_t> rows(n * bits), rows_rv(n * bits_rv);
        CHECK(zkaes_chunk_public_inputs(kind, n, h0, c.get(), len, tg, tag_len, st, rows.data(), &bits) == 0, "%s", zkaes_last_error());
        CHECK(zkaes_chunk_public_inputs_rv(kind, n, h0, c.get(), len, tg, tag_len, st, m.get(), len / 8, r.get(), rows_rv.data(), &bits_rv) == 0, "%s", zkaes_last_error());
        for (size_t j = 0; j < n; j++) {
            CHECK(zk::chunk_mask_slice(mask.data(), j, chunk) == mask.data() + chunk * j / 8, "slice %zu", j);
            std::vector<uint8_t> want(rows.begin() + j * bits, rows.begin() + (j + 1) * bits), mb = bits_of(zk::chunk_mask_slice(mask.data(), j, chunk), zk::mask_bytes(chunk)), rb = bits_of(revealed.data() + chunk * j, chunk);
            want.insert(want.end(), mb.begin(), mb.end());
            want.insert(want.end(), rb.begin(), rb.end());
            CHECK(std::vector<uint8_t>(rows_rv.begin() + j * bits_rv, rows_rv.begin() + (j + 1) * bits_rv) == want, "kind %d chunk %zu n %zu row %zu", kind, chunk, n, j);
            cases++;
        }
        // a revealed byte that the mask hides must be an error, not a row
        std::vector<uint8_t> bad_mask(mask), bad_rev(revealed);
        bad_mask[0] &= 0xfe; bad_rev[0] = 1;
        CHECK(zkaes_chunk_public_inputs_rv(kind, n, h0, c.get(), len, tg, tag_len, st, bad_mask.data(), len / 8, bad_rev.data(), nullptr, &bits_rv) != 0, "revealed under a zero mask bit");
        CHECK(zkaes_chunk_public_inputs_rv(kind, n, h0, c.get(), len, tg, tag_len, st, m.get(), len / 8 + 1, r.get(), nullptr, &bits_rv) != 0, "mask length");
        CHECK(zkaes_chunk_public_inputs_rv(kind, n, h0, c.get(), len, tg, tag_len, st, nullptr, len / 8, r.get(), nullptr, &bits_rv) != 0, "no mask");
    }
    CHECK(cases == 3 * 2 * (1 + 2 + 3) * 2 * 2, "%zu", cases);
    // ---- the lone CTR slice that is no whole block: 17 bytes, 3 mask bytes, the 7 bits beyond the length must be zero
    const std::vector<uint8_t> ct17 = stream(17, 99), msg17 = stream(17, 98), icb = stream(16, 97);
    uint8_t mask17[3] = {0x81, 0x80, 0x01}, rev17[17], out17[17];
    zk::reveal_bytes(msg17.data(), mask17, 17, rev17);
    CHECK(zk::mask_bytes(17) == 3 && zk::mask_bytes(16) == 2 && zk::mask_bytes(1) == 1, "mask bytes");
    CHECK(rev17[0] == msg17[0] && rev17[7] == msg17[7] && rev17[15] == msg17[15] && rev17[16] == msg17[16] && rev17[1] == 0 && rev17[8] == 0, "by hand");
    size_t bits = 0;
    CHECK(zkaes_chunk_public_inputs_rv(ZKAES_CIRCUIT_AES_CTR, 1, icb.data(), ct17.data(), 17, nullptr, 0, nullptr, mask17, 3, rev17, nullptr, &bits) == 0 && bits == 128 + 136 + 24 + 136, "lone CTR row");
    mask17[2] = 0x03;
    CHECK(zkaes_chunk_public_inputs_rv(ZKAES_CIRCUIT_AES_CTR, 1, icb.data(), ct17.data(), 17, nullptr, 0, nullptr, mask17, 3, rev17, nullptr, &bits) != 0, "a mask bit at the length");
    CHECK(zkaes_reveal_bytes(msg17.data(), 17, mask17, 3, out17) != 0, "a mask bit at the length");
    mask17[2] = 0x80;
    CHECK(zkaes_reveal_bytes(msg17.data(), 17, mask17, 3, out17) != 0, "the last mask bit");
    mask17[2] = 0x01;
    CHECK(zkaes_reveal_bytes(msg17.data(), 17, mask17, 2, out17) != 0 && zkaes_reveal_bytes(msg17.data(), 17, nullptr, 3, out17) != 0 && zkaes_reveal_bytes(msg17.data(), 17, mask17, 3, out17) == 0 && memcmp(out17, rev17, 17) == 0, "zkaes_reveal_bytes arguments");
    if (failures) { printf("reveal_statement_check: %d failure(s)\n", failures); return 1; }
    printf("reveal_statement_check ok\n");
    return 0;
}
