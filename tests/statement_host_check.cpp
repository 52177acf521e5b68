// tests/statement_host_check.cpp -- the chunk-header rule on both of its sides, stand-alone, host only (built under ASan + UBSan by tests/test_statement_host.py with
// circuit.cpp, marlin_codec.cpp and capi_host.cpp; nothing is loaded into python).  The prover reaches the rule as zk::chunk_mode_header (csrc/statement.hpp), a
// verifier as row j of zkaes_chunk_public_inputs: the first header bits of row j must be the bits of chunk_mode_header(j), for ECB, CBC and CTR, slices of 16 and 32
// bytes, 1, 2 and 3 chunks, no key tag, 16 and 32 tag bytes, with and without states -- and both must be what is written out by hand below.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "statement.hpp"
#include "../include/zkaes.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

// 8 bits per byte, LSB first, one byte (0/1) each: the public-input encoding
static std::vector<uint8_t> bits_of(const uint8_t *bytes, size_t n) {
    std::vector<uint8_t> out;
    for (size_t i = 0; i < n; i++) for (int b = 0; b < 8; b++) out.push_back((bytes[i] >> b) & 1);
    return out;
}
static void append(std::vector<uint8_t> &to, const std::vector<uint8_t> &from) { to.insert(to.end(), from.begin(), from.end()); }
static std::vector<uint8_t> stream(size_t n, uint32_t seed) {
    std::vector<uint8_t> out(n);
    for (size_t i = 0; i < n; i++) { seed = seed * 1664525u + 1013904223u; out[i] = (uint8_t)(seed >> 24); }
    return out;
}
// the rows of the C ABI; empty when the call fails
static std::vector<std::vector<uint8_t>> rows_of(int kind, size_t n_chunks, const uint8_t *hdr0, const std::vector<uint8_t> &ct, const uint8_t *key_tag, size_t key_tag_len, const uint8_t *states) {
    size_t n_bits = 0;
    if (zkaes_chunk_public_inputs(kind, n_chunks, hdr0, ct.data(), ct.size(), key_tag, key_tag_len, states, nullptr, &n_bits) != 0) { printf("%s\n", zkaes_last_error()); return {}; }
    std::vector<uint8_t> flat(n_chunks * n_bits);
    if (zkaes_chunk_public_inputs(kind, n_chunks, hdr0, ct.data(), ct.size(), key_tag, key_tag_len, states, flat.data(), &n_bits) != 0) { printf("%s\n", zkaes_last_error()); return {}; }
    std::vector<std::vector<uint8_t>> rows;
    for (size_t j = 0; j < n_chunks; j++) rows.emplace_back(flat.begin() + j * n_bits, flat.begin() + (j + 1) * n_bits);
    return rows;
}
// both sides against a header written by hand
static void expect_header(const char *what, int kind, size_t j, size_t chunk, size_t n_chunks, const uint8_t *hdr0, const std::vector<uint8_t> &ct, const uint8_t want[16]) {
    uint8_t got[16];
    memset(got, 0xA5, 16);
    CHECK(zk::chunk_mode_header(kind, j, chunk, hdr0, ct.data(), got) == 16, "%s", what);
    CHECK(memcmp(got, want, 16) == 0, "%s: chunk_mode_header(%zu)", what, j);
    std::vector<std::vector<uint8_t>> rows = rows_of(kind, n_chunks, hdr0, ct, nullptr, 0, nullptr);
    CHECK(rows.size() == n_chunks, "%s", what);
    if (rows.size() != n_chunks) return;
    std::vector<uint8_t> row = bits_of(want, 16);
    append(row, bits_of(ct.data() + chunk * j, chunk));
    CHECK(rows[j] == row, "%s: row %zu of zkaes_chunk_public_inputs", what, j);
}

int main() {
    const int kinds[3] = {ZKAES_CIRCUIT_AES, ZKAES_CIRCUIT_AES_CBC, ZKAES_CIRCUIT_AES_CTR};
    size_t cases = 0;
    for (int kind : kinds) for (size_t chunk : {(size_t)16, (size_t)32}) for (size_t n_chunks : {(size_t)1, (size_t)2, (size_t)3})
        for (size_t tag_len : {(size_t)0, (size_t)16, (size_t)32}) for (int with_states = 0; with_states < 2; with_states++) {
            const uint32_t seed = (uint32_t)(kind * 1000 + chunk * 100 + n_chunks * 10 + tag_len + with_states);
            const std::vector<uint8_t> ct = stream(chunk * n_chunks, seed), tag = stream(32, seed + 1), states = stream(32 * (n_chunks + 1), seed + 2);
            std::vector<uint8_t> hdr0 = stream(16, seed + 3);
            if (kind == ZKAES_CIRCUIT_AES_CTR) memset(hdr0.data() + 8, 0xff, 8);                  // every CTR case carries out of the low half
            const uint8_t *h0 = kind == ZKAES_CIRCUIT_AES ? nullptr : hdr0.data();
            std::vector<std::vector<uint8_t>> rows = rows_of(kind, n_chunks, h0, ct, tag_len ? tag.data() : nullptr, tag_len, with_states ? states.data() : nullptr);
            CHECK(rows.size() == n_chunks, "kind %d chunk %zu n %zu", kind, chunk, n_chunks);
            if (rows.size() != n_chunks) continue;
            for (size_t j = 0; j < n_chunks; j++) {
                uint8_t hdr[16];
                const size_t hb = zk::chunk_mode_header(kind, j, chunk, h0, ct.data(), hdr);
                CHECK(hb == (kind == ZKAES_CIRCUIT_AES ? 0u : 16u), "kind %d", kind);
                std::vector<uint8_t> want = bits_of(hdr, hb);
                append(want, bits_of(ct.data() + chunk * j, chunk));
                append(want, bits_of(tag.data(), tag_len));
                if (with_states) append(want, bits_of(states.data() + 32 * j, 64));
                CHECK(rows[j].size() == 8 * hb + 8 * chunk + 8 * tag_len + (with_states ? 512 : 0), "kind %d chunk %zu n %zu tag %zu states %d", kind, chunk, n_chunks, tag_len, with_states);
                CHECK(rows[j] == want, "kind %d chunk %zu n %zu tag %zu states %d row %zu", kind, chunk, n_chunks, tag_len, with_states, j);
                cases++;
            }
        }
    CHECK(cases == 3 * 2 * (1 + 2 + 3) * 3 * 2, "%zu", cases);

    // ---- by hand.  CBC: chunk j > 0 enters under the ciphertext block ahead of its slice, chunk 0 under the iv
    std::vector<uint8_t> ct(96);
    for (size_t i = 0; i < ct.size(); i++) ct[i] = (uint8_t)i;
    const uint8_t iv[16] = {0xf0, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa, 0xfb, 0xfc, 0xfd, 0xfe, 0xff};
    const uint8_t block0[16] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
    const uint8_t block1[16] = {16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31};
    const uint8_t block3[16] = {48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63};
    std::vector<uint8_t> ct48(ct.begin(), ct.begin() + 48);
    expect_header("CBC 16 x 3, chunk 0", ZKAES_CIRCUIT_AES_CBC, 0, 16, 3, iv, ct48, iv);
    expect_header("CBC 16 x 3, chunk 1", ZKAES_CIRCUIT_AES_CBC, 1, 16, 3, iv, ct48, block0);
    expect_header("CBC 16 x 3, chunk 2", ZKAES_CIRCUIT_AES_CBC, 2, 16, 3, iv, ct48, block1);
    expect_header("CBC 32 x 3, chunk 1", ZKAES_CIRCUIT_AES_CBC, 1, 32, 3, iv, ct, block1);
    expect_header("CBC 32 x 3, chunk 2", ZKAES_CIRCUIT_AES_CBC, 2, 32, 3, iv, ct, block3);
    // CTR: icb + j x the chunk's blocks, the 16 bytes one big-endian integer mod 2^128
    uint8_t all_ff[16], zero[16] = {0};
    memset(all_ff, 0xff, 16);
    std::vector<uint8_t> ct32(ct.begin(), ct.begin() + 32);
    expect_header("CTR from ff x 16, chunk 0", ZKAES_CIRCUIT_AES_CTR, 0, 16, 2, all_ff, ct32, all_ff);
    expect_header("CTR from ff x 16 wraps to zero at chunk 1", ZKAES_CIRCUIT_AES_CTR, 1, 16, 2, all_ff, ct32, zero);
    const uint8_t low_ff[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff};
    const uint8_t carried[16] = {0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0};
    const uint8_t carried_1[16] = {0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1};
    expect_header("CTR from 00 x 8 | ff x 8: the carry crosses byte 8", ZKAES_CIRCUIT_AES_CTR, 1, 16, 2, low_ff, ct32, carried);
    expect_header("CTR from 00 x 8 | ff x 8, two blocks per chunk", ZKAES_CIRCUIT_AES_CTR, 1, 32, 3, low_ff, ct, carried_1);
    // the lone CTR slice that is no whole block: one chunk of 17 bytes under the icb itself
    std::vector<uint8_t> ct17(ct.begin(), ct.begin() + 17);
    expect_header("CTR lone 17 bytes", ZKAES_CIRCUIT_AES_CTR, 0, 17, 1, low_ff, ct17, low_ff);
    std::vector<std::vector<uint8_t>> lone = rows_of(ZKAES_CIRCUIT_AES_CTR, 1, low_ff, ct17, nullptr, 0, nullptr);
    CHECK(lone.size() == 1 && lone[0].size() == 128 + 8 * 17, "lone CTR row");
    std::vector<uint8_t> ct34(ct.begin(), ct.begin() + 34);
    size_t n_bits = 0;
    CHECK(zkaes_chunk_public_inputs(ZKAES_CIRCUIT_AES_CTR, 2, low_ff, ct34.data(), 34, nullptr, 0, nullptr, nullptr, &n_bits) != 0, "two slices of 17 bytes must be refused");
    // ECB has no header: nothing is written
    uint8_t untouched[16];
    memset(untouched, 0xA5, 16);
    CHECK(zk::chunk_mode_header(ZKAES_CIRCUIT_AES, 1, 16, nullptr, ct.data(), untouched) == 0 && untouched[0] == 0xA5 && untouched[15] == 0xA5, "ECB");
    if (failures) { printf("statement_host_check: %d failure(s)\n", failures); return 1; }
    printf("statement_host_check ok\n");
    return 0;
}
