// tests/digest_host_check.cpp -- stand-alone check of the host-only plaintext-digest entry points of include/zkaes.h, built by tests/test_digest_host.py with
// -fsanitize=address,undefined together with csrc/circuit.cpp, csrc/marlin_codec.cpp and csrc/capi_host.cpp (no HIP, no GPU):
//   * zkaes_sha256_finish for FIPS 180-4's "abc" and the empty message, into and from heap buffers of exactly their size; zkaes_sha256_chain then zkaes_sha256_finish over
//     a split message equals the one-shot digest; lengths that are no multiple of 64, a ragged prefix and null arguments are errors;
//   * zkaes_circuit_info_pd at digest kind 0 equals zkaes_circuit_info_kt, grows by 512 instance variables with a digest, refuses kind 3, a chain key whose length is no
//     multiple of 64, a prefix on a chain key, a ragged prefix and a digest on an ops circuit;
//   * zkaes_verify_digest_chunked and zkaes_verify_encryption_gcm_digest, fed the committed ECB verifying key and proof: the key as stored (it knows its 128 public bits:
//     every digest shape is an error), after the ark transport (|X| = 256: no digest shape fits, every chunk is rejected), and the ark image with |X| patched to 1024,
//     which the 16-byte ECB statement with two states does fit -- there the proof is parsed and checked, whole, truncated at every length and as garbage, one and two
//     chunks, with and without a key tag: a chunk that does not parse is a rejected chunk, not an error.  Nothing is ever accepted.
// usage: digest_host_check <directory of the golden fixtures>.  Prints "digest_host_check ok" and exits 0, or says what went wrong and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "../include/zkaes.h"

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, zkaes_last_error()); fails++; } } while (0)

static std::vector<uint8_t> slurp(const std::string &path) {
    std::vector<uint8_t> v;
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path.c_str()); exit(1); }
    uint8_t buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}
// a heap copy of exactly n bytes: the sanitizer watches both ends
static std::unique_ptr<uint8_t[]> exact(const uint8_t *src, size_t n) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[n ? n : 1]);
    if (n) memcpy(p.get(), src, n);
    return p;
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s <golden dir>\n", argv[0]); return 1; }
    const std::string gold = argv[1];
    // ---- the hash (FIPS 180-4 appendix B.1; the empty message)
    const uint8_t abc_digest[32] = {0xba, 0x78, 0x16, 0xbf, 0x8f, 0x01, 0xcf, 0xea, 0x41, 0x41, 0x40, 0xde, 0x5d, 0xae, 0x22, 0x23, 0xb0, 0x03, 0x61, 0xa3, 0x96, 0x17, 0x7a, 0x9c, 0xb4, 0x10, 0xff, 0x61, 0xf2, 0x00, 0x15, 0xad};
    const uint8_t empty_digest[32] = {0xe3, 0xb0, 0xc4, 0x42, 0x98, 0xfc, 0x1c, 0x14, 0x9a, 0xfb, 0xf4, 0xc8, 0x99, 0x6f, 0xb9, 0x24, 0x27, 0xae, 0x41, 0xe4, 0x64, 0x9b, 0x93, 0x4c, 0xa4, 0x95, 0x99, 0x1b, 0x78, 0x52, 0xb8, 0x55};
    {
        auto abc = exact((const uint8_t *)"abc", 3);
        std::unique_ptr<uint8_t[]> out(new uint8_t[32]);
        CHECK(zkaes_sha256_finish(nullptr, 0, abc.get(), 3, out.get()) == 0 && memcmp(out.get(), abc_digest, 32) == 0);
        CHECK(zkaes_sha256_finish(nullptr, 0, nullptr, 0, out.get()) == 0 && memcmp(out.get(), empty_digest, 32) == 0);
        uint8_t seq[200];
        for (int i = 0; i < 200; i++) seq[i] = (uint8_t)(3 * i + 1);
        for (size_t len : {(size_t)64, (size_t)65, (size_t)119, (size_t)120, (size_t)128, (size_t)200}) {
            auto m = exact(seq, len);
            const size_t head = len / 64 * 64 == len ? len - 64 : len / 64 * 64;
            uint8_t whole[32], mid[32], split[32];
            CHECK(zkaes_sha256_finish(nullptr, 0, m.get(), len, whole) == 0);
            CHECK(zkaes_sha256_chain(nullptr, m.get(), head, mid) == 0);
            auto tail = exact(seq + head, len - head);
            CHECK(zkaes_sha256_finish(mid, head, tail.get(), len - head, split) == 0 && memcmp(whole, split, 32) == 0);
        }
        uint8_t st[32];
        CHECK(zkaes_sha256_chain(nullptr, seq, 63, st) != 0);
        CHECK(zkaes_sha256_chain(nullptr, nullptr, 64, st) != 0);
        CHECK(zkaes_sha256_chain(nullptr, seq, 64, nullptr) != 0);
        CHECK(zkaes_sha256_finish(nullptr, 32, seq, 3, st) != 0);
        CHECK(zkaes_sha256_finish(nullptr, (uint64_t)1 << 61, seq, 3, st) != 0);
        CHECK(zkaes_sha256_finish(nullptr, 0, nullptr, 3, st) != 0);
        CHECK(zkaes_sha256_finish(nullptr, 0, seq, 3, nullptr) != 0);
    }
    // ---- circuit queries
    {
        uint64_t a[12], b[12];
        CHECK(zkaes_circuit_info_kt(ZKAES_CIRCUIT_AES, 128, 1, 16, 0, a) == 0 && zkaes_circuit_info_pd(ZKAES_CIRCUIT_AES, 128, 1, ZKAES_DIGEST_NONE, 0, 16, 0, b) == 0 && memcmp(a, b, sizeof a) == 0);
        CHECK(zkaes_circuit_info_pd(ZKAES_CIRCUIT_AES, 128, 1, ZKAES_DIGEST_FINAL, 64, 16, 0, b) == 0 && b[1] == a[1] + 512);
        CHECK(zkaes_circuit_info_pd(ZKAES_CIRCUIT_AES, 128, 0, 3, 0, 64, 0, b) != 0);
        CHECK(zkaes_circuit_info_pd(ZKAES_CIRCUIT_AES, 128, 0, ZKAES_DIGEST_CHAIN, 0, 16, 0, b) != 0);
        CHECK(zkaes_circuit_info_pd(ZKAES_CIRCUIT_AES, 128, 0, ZKAES_DIGEST_CHAIN, 64, 64, 0, b) != 0);
        CHECK(zkaes_circuit_info_pd(ZKAES_CIRCUIT_AES, 128, 0, ZKAES_DIGEST_NONE, 64, 64, 0, b) != 0);
        CHECK(zkaes_circuit_info_pd(ZKAES_CIRCUIT_AES, 128, 0, ZKAES_DIGEST_FINAL, 32, 16, 0, b) != 0);
        CHECK(zkaes_circuit_info_pd(ZKAES_CIRCUIT_AES, 128, 0, ZKAES_DIGEST_FINAL, (uint64_t)1 << 61, 16, 0, b) != 0);
        CHECK(zkaes_circuit_info_pd(ZKAES_CIRCUIT_OPS_XOR, 128, 0, ZKAES_DIGEST_FINAL, 0, 0, 0, b) != 0);
        uint64_t rows = 0, nnz = 0;
        CHECK(zkaes_circuit_matrix_pd(ZKAES_CIRCUIT_AES, 128, 0, 3, 0, 16, 0, 0, &rows, &nnz, nullptr, nullptr, nullptr) != 0);
    }
    // ---- the ECB fixtures through the digest verifiers
    const std::vector<uint8_t> vkb = slurp(gold + "/gpu_aes16_vk.bin"), proof = slurp(gold + "/gpu_aes16_proof.bin");
    const uint8_t ecb_ct32[32] = {0x39, 0x25, 0x84, 0x1d, 0x02, 0xdc, 0x09, 0xfb, 0xdc, 0x11, 0x85, 0x97, 0x19, 0x6a, 0x0b, 0x32,         // FIPS-197 appendix B: what the fixture proves under ECB,
                                  0x39, 0x25, 0x84, 0x1d, 0x02, 0xdc, 0x09, 0xfb, 0xdc, 0x11, 0x85, 0x97, 0x19, 0x6a, 0x0b, 0x32};        // twice (a two-chunk ciphertext)
    const uint8_t iv[16] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
    uint8_t zero96[96] = {0};
    zkaes_vk *vk = nullptr, *vk_ark = nullptr, *vk_1024 = nullptr;
    CHECK(zkaes_vk_deserialize(vkb.data(), vkb.size(), &vk) == 0 && vk);
    if (!vk) return 1;
    {
        uint8_t *ark = nullptr; size_t ark_len = 0;
        CHECK(zkaes_vk_serialize_ark(vk, &ark, &ark_len) == 0 && ark && ark_len > 32);
        CHECK(zkaes_vk_deserialize_ark(ark, ark_len, &vk_ark) == 0 && vk_ark);
        uint64_t ninst = 0;
        for (int i = 0; i < 8; i++) ninst |= (uint64_t)ark[24 + i] << (8 * i);
        CHECK(ninst == 256);                                                                    // index info: variables, constraints, non-zeros, instance variables
        ark[25] = 0x04; ark[24] = 0x00;                                                         // |X| = 1024: the shape of a 16-byte ECB statement with H_in and H_out
        CHECK(zkaes_vk_deserialize_ark(ark, ark_len, &vk_1024) == 0 && vk_1024);
        zkaes_bytes_free(ark);
    }
    if (!vk_ark || !vk_1024) return 1;
    int acc = 7, each[2] = {7, 7};
    size_t n_acc = 7, lens[2] = {proof.size(), proof.size()};
    std::vector<uint8_t> two(proof);
    two.insert(two.end(), proof.begin(), proof.end());
    CHECK(zkaes_verify_encryption(vk, proof.data(), proof.size(), ecb_ct32, 16, &acc) == 0 && acc == 1);            // (the fixtures are what they claim to be)
    auto tag16 = exact(zero96, 16), ct16 = exact(ecb_ct32, 16), ct32 = exact(ecb_ct32, 32), ct17 = exact(ecb_ct32, 17), st2 = exact(zero96, 64), st3 = exact(zero96, 96);
    for (int tagged = 0; tagged < 2; tagged++) {
        const uint8_t *tg = tagged ? tag16.get() : nullptr;
        const size_t tl = tagged ? 16 : 0;
        // the stored key knows its 128 public bits: with 512 digest bits behind them no shape fits, every call is an error and nothing is accepted
        each[0] = each[1] = 7; n_acc = 7;
        CHECK(zkaes_verify_digest_chunked(vk, ZKAES_CIRCUIT_AES, proof.data(), lens, 1, nullptr, ct16.get(), 16, tg, tl, st2.get(), each, &n_acc) != 0 && each[0] == 0 && n_acc == 0);
        CHECK(zkaes_verify_digest_chunked(vk, ZKAES_CIRCUIT_AES, two.data(), lens, 2, nullptr, ct32.get(), 32, tg, tl, st3.get(), each, &n_acc) != 0 && each[0] == 0 && each[1] == 0 && n_acc == 0);
        CHECK(zkaes_verify_digest_chunked(vk, ZKAES_CIRCUIT_AES_CBC, proof.data(), lens, 1, iv, ct16.get(), 16, tg, tl, st2.get(), each, &n_acc) != 0 && n_acc == 0);
        CHECK(zkaes_verify_digest_chunked(vk, ZKAES_CIRCUIT_AES_CTR, proof.data(), lens, 1, iv, ct17.get(), 17, tg, tl, st2.get(), each, &n_acc) != 0 && n_acc == 0);
        acc = 7;
        CHECK(zkaes_verify_encryption_gcm_digest(vk, proof.data(), proof.size(), iv, nullptr, 0, ct17.get(), 17, iv, tg, tl, nullptr, st2.get(), &acc) != 0 && acc == 0);
        // the transported key knows |X| = 256 only, and every digest shape has more than 511 inputs: rejected, not an error
        each[0] = each[1] = 7; n_acc = 7;
        CHECK(zkaes_verify_digest_chunked(vk_ark, ZKAES_CIRCUIT_AES, two.data(), lens, 2, nullptr, ct32.get(), 32, tg, tl, st3.get(), each, &n_acc) == 0 && each[0] == 0 && each[1] == 0 && n_acc == 0);
        acc = 7;
        CHECK(zkaes_verify_encryption_gcm_digest(vk_ark, proof.data(), proof.size(), iv, nullptr, 0, ct17.get(), 1, iv, tg, tl, nullptr, st2.get(), &acc) == 0 && acc == 0);
        // |X| = 1024: the 16-byte ECB statement with two states (and a 16-byte tag) fits, so the proof is parsed and checked -- and fails
        each[0] = each[1] = 7; n_acc = 7;
        CHECK(zkaes_verify_digest_chunked(vk_1024, ZKAES_CIRCUIT_AES, proof.data(), lens, 1, nullptr, ct16.get(), 16, tg, tl, st2.get(), each, &n_acc) == 0 && each[0] == 0 && n_acc == 0);
        CHECK(zkaes_verify_digest_chunked(vk_1024, ZKAES_CIRCUIT_AES, two.data(), lens, 2, nullptr, ct32.get(), 32, tg, tl, st3.get(), each, &n_acc) == 0 && each[0] == 0 && each[1] == 0 && n_acc == 0);
        CHECK(zkaes_verify_digest_chunked(vk_1024, ZKAES_CIRCUIT_AES, two.data(), lens, 2, nullptr, ct32.get(), 32, tg, tl, st3.get(), nullptr, nullptr) == 0);
        CHECK(zkaes_verify_digest_chunked(vk_1024, ZKAES_CIRCUIT_AES_CBC, proof.data(), lens, 1, iv, ct16.get(), 16, tg, tl, st2.get(), each, &n_acc) == 0 && each[0] == 0);
        CHECK(zkaes_verify_digest_chunked(vk_1024, ZKAES_CIRCUIT_AES_CTR, proof.data(), lens, 1, iv, ct17.get(), 17, tg, tl, st2.get(), each, &n_acc) == 0 && each[0] == 0);      // ragged lone CTR
        acc = 7;
        CHECK(zkaes_verify_encryption_gcm_digest(vk_1024, proof.data(), proof.size(), iv, nullptr, 0, ct16.get(), 1, iv, tg, tl, nullptr, st2.get(), &acc) == 0 && acc == 0);
        acc = 7;
        CHECK(zkaes_verify_encryption_gcm_digest(vk_1024, proof.data(), proof.size(), iv, nullptr, 0, ct16.get(), 1, iv, tg, tl, st2.get(), st2.get() + 32, &acc) == 0 && acc == 0);
    }
    // arguments that do not go together: errors, whatever the key
    for (zkaes_vk *k : {vk, vk_ark, vk_1024}) {
        for (size_t tl : {(size_t)0, (size_t)15, (size_t)17, (size_t)48}) {                        // a key tag of a length that is none (0 goes with NULL only)
            CHECK(zkaes_verify_digest_chunked(k, ZKAES_CIRCUIT_AES, proof.data(), lens, 1, nullptr, ct16.get(), 16, tag16.get(), tl, st2.get(), each, &n_acc) != 0 && n_acc == 0);
            acc = 7;
            CHECK(zkaes_verify_encryption_gcm_digest(k, proof.data(), proof.size(), iv, nullptr, 0, ct16.get(), 16, iv, tag16.get(), tl, nullptr, st2.get(), &acc) != 0 && acc == 0);
        }
        CHECK(zkaes_verify_digest_chunked(k, ZKAES_CIRCUIT_AES, proof.data(), lens, 1, nullptr, ct16.get(), 16, nullptr, 16, st2.get(), each, &n_acc) != 0);
        CHECK(zkaes_verify_digest_chunked(k, ZKAES_CIRCUIT_AES_GCM, proof.data(), lens, 1, nullptr, ct16.get(), 16, nullptr, 0, st2.get(), each, &n_acc) != 0);
        CHECK(zkaes_verify_digest_chunked(k, ZKAES_CIRCUIT_OPS_XOR, proof.data(), lens, 1, nullptr, ct16.get(), 16, nullptr, 0, st2.get(), each, &n_acc) != 0);
        CHECK(zkaes_verify_digest_chunked(k, ZKAES_CIRCUIT_AES, proof.data(), lens, 1, iv, ct16.get(), 16, nullptr, 0, st2.get(), each, &n_acc) != 0);
        CHECK(zkaes_verify_digest_chunked(k, ZKAES_CIRCUIT_AES_CBC, proof.data(), lens, 1, nullptr, ct16.get(), 16, nullptr, 0, st2.get(), each, &n_acc) != 0);
        CHECK(zkaes_verify_digest_chunked(k, ZKAES_CIRCUIT_AES, proof.data(), lens, 0, nullptr, ct16.get(), 16, nullptr, 0, st2.get(), nullptr, &n_acc) != 0);
        CHECK(zkaes_verify_digest_chunked(k, ZKAES_CIRCUIT_AES, proof.data(), lens, 1, nullptr, ct16.get(), 0, nullptr, 0, st2.get(), each, &n_acc) != 0);
        CHECK(zkaes_verify_digest_chunked(k, ZKAES_CIRCUIT_AES, proof.data(), lens, 1, nullptr, ct17.get(), 17, nullptr, 0, st2.get(), each, &n_acc) != 0);
        CHECK(zkaes_verify_digest_chunked(k, ZKAES_CIRCUIT_AES_CTR, two.data(), lens, 2, iv, ct32.get(), 30, nullptr, 0, st3.get(), each, &n_acc) != 0);      // two ragged CTR chunks
        CHECK(zkaes_verify_digest_chunked(k, ZKAES_CIRCUIT_AES, proof.data(), lens, 1, nullptr, ct16.get(), 16, nullptr, 0, nullptr, each, &n_acc) != 0);
        CHECK(zkaes_verify_digest_chunked(k, ZKAES_CIRCUIT_AES, nullptr, lens, 1, nullptr, ct16.get(), 16, nullptr, 0, st2.get(), each, &n_acc) != 0);
        CHECK(zkaes_verify_encryption_gcm_digest(k, proof.data(), proof.size(), iv, nullptr, 0, ct16.get(), 0, iv, nullptr, 0, nullptr, st2.get(), &acc) != 0);
        CHECK(zkaes_verify_encryption_gcm_digest(k, proof.data(), proof.size(), iv, nullptr, 0, ct16.get(), 16, iv, nullptr, 0, nullptr, nullptr, &acc) != 0);
    }
    for (size_t cut = 0; cut < proof.size(); cut++) {                                           // every truncation, in a heap buffer of exactly that size, as chunk 0 of two: chunk 1 is
        const bool whole = cut % 96 == 0;                                                       // the whole proof (parsed and checked) now and then, else one byte that does not parse
        const size_t second = whole ? proof.size() : 1;
        std::vector<uint8_t> t(proof.begin(), proof.begin() + cut);
        t.insert(t.end(), proof.begin(), proof.begin() + second);
        auto buf = exact(t.data(), t.size());
        size_t l2[2] = {cut, second};
        each[0] = each[1] = 7; n_acc = 7;
        CHECK(zkaes_verify_digest_chunked(vk_1024, ZKAES_CIRCUIT_AES, buf.get(), l2, 2, nullptr, ct32.get(), 32, nullptr, 0, st3.get(), each, &n_acc) == 0 && each[0] == 0 && each[1] == 0 && n_acc == 0);
        auto lone = exact(proof.data(), cut);
        acc = 7;
        CHECK(zkaes_verify_encryption_gcm_digest(vk_1024, lone.get(), cut, iv, nullptr, 0, ct16.get(), 1, iv, nullptr, 0, nullptr, st2.get(), &acc) != 0 && acc == 0);      // (the lone GCM form reports a proof that does not parse)
    }
    srand(0xd16);
    for (int round = 0; round < 24; round++) {                                                  // garbage of the proof's length, and the proof with one byte changed
        std::vector<uint8_t> g(proof);
        if (round & 1) for (auto &b : g) b = (uint8_t)rand(); else g[(size_t)rand() % g.size()] ^= (uint8_t)(1 + rand() % 255);
        auto buf = exact(g.data(), g.size());
        each[0] = 7; n_acc = 7;
        CHECK(zkaes_verify_digest_chunked(vk_1024, ZKAES_CIRCUIT_AES, buf.get(), lens, 1, nullptr, ct16.get(), 16, nullptr, 0, st2.get(), each, &n_acc) == 0 && each[0] == 0 && n_acc == 0);
    }
    zkaes_vk_free(vk);
    zkaes_vk_free(vk_ark);
    zkaes_vk_free(vk_1024);
    if (fails) { fprintf(stderr, "digest_host_check: %d failure(s)\n", fails); return 1; }
    printf("digest_host_check ok\n");
    return 0;
}
