// tests/reveal_host_check.cpp -- stand-alone check of the host-only selective-disclosure entry points of include/zkaes.h, built by
// tests/test_reveal_host.py with -fsanitize=address,undefined together with csrc/circuit.cpp, csrc/marlin_codec.cpp and csrc/capi_host.cpp (no HIP, no GPU):
//   * zkaes_circuit_info_rv at reveal 0 equals zkaes_circuit_info_pd, grows by 8 ceil(L / 8) + 8 L instance variables and no witness with reveal 1, refuses reveal 2 and
//     the ops kinds; zkaes_circuit_matrix_rv refuses the same;
//   * zkaes_verify_reveal_chunked, zkaes_verify_encryption_gcm_reveal and zkaes_chunk_public_inputs_rv refuse, as ERRORS whatever the key, a mask bit at or beyond the
//     length and a non-zero revealed byte under a zero mask bit;
//   * the two verifiers, fed the committed ECB verifying key and proof: the key as stored (it knows its 128 public bits: every reveal shape is an error), after the ark
//     transport (|X| = 256: no reveal shape fits, every chunk is rejected), and the ark image with |X| patched to 512, which the 16-byte ECB reveal statement does fit --
//     there the proof is parsed and checked, whole, truncated at every length and as garbage, one and two chunks: a chunk that does not parse is a rejected chunk, not an
//     error.  Nothing is ever accepted.
// usage: reveal_host_check <directory of the golden fixtures>.  Prints "reveal_host_check ok" and exits 0, or says what went wrong and exits 1.
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
    // ---- circuit queries
    {
        uint64_t a[12], b[12];
        CHECK(zkaes_circuit_info_pd(ZKAES_CIRCUIT_AES, 128, 1, ZKAES_DIGEST_NONE, 0, 16, 0, a) == 0 && zkaes_circuit_info_rv(ZKAES_CIRCUIT_AES, 128, 1, ZKAES_DIGEST_NONE, 0, 0, 16, 0, b) == 0 && memcmp(a, b, sizeof a) == 0);
        CHECK(zkaes_circuit_info_rv(ZKAES_CIRCUIT_AES, 128, 1, ZKAES_DIGEST_NONE, 0, 1, 16, 0, b) == 0 && b[1] == a[1] + 16 + 128 && b[2] == a[2] && b[0] == a[0] + 17 * 16);
        CHECK(zkaes_circuit_info_pd(ZKAES_CIRCUIT_AES_CTR, 128, 0, ZKAES_DIGEST_FINAL, 0, 17, 0, a) == 0 && zkaes_circuit_info_rv(ZKAES_CIRCUIT_AES_CTR, 128, 0, ZKAES_DIGEST_FINAL, 0, 1, 17, 0, b) == 0 &&
              b[1] == a[1] + 24 + 136 && b[2] == a[2] && b[0] == a[0] + 16 * 3 + 15 * 17);
        CHECK(zkaes_circuit_info_rv(ZKAES_CIRCUIT_AES, 128, 0, ZKAES_DIGEST_NONE, 0, 2, 16, 0, b) != 0);
        CHECK(zkaes_circuit_info_rv(ZKAES_CIRCUIT_OPS_XOR, 128, 0, ZKAES_DIGEST_NONE, 0, 1, 0, 0, b) != 0);
        CHECK(zkaes_circuit_info_rv(ZKAES_CIRCUIT_OPS_ADD, 128, 0, ZKAES_DIGEST_NONE, 0, 1, 0, 0, b) != 0);
        CHECK(zkaes_circuit_info_rv(6, 128, 0, ZKAES_DIGEST_NONE, 0, 1, 16, 0, b) != 0);                 // a GCM segment circuit has no reveal form
        uint64_t rows = 0, nnz = 0;
        CHECK(zkaes_circuit_matrix_rv(ZKAES_CIRCUIT_AES, 128, 0, ZKAES_DIGEST_NONE, 0, 2, 16, 0, 0, &rows, &nnz, nullptr, nullptr, nullptr) != 0);
        CHECK(zkaes_circuit_matrix_rv(ZKAES_CIRCUIT_OPS_XOR, 128, 0, ZKAES_DIGEST_NONE, 0, 1, 0, 0, 0, &rows, &nnz, nullptr, nullptr, nullptr) != 0);
    }
    // ---- the ECB fixtures through the reveal verifiers
    const std::vector<uint8_t> vkb = slurp(gold + "/gpu_aes16_vk.bin"), proof = slurp(gold + "/gpu_aes16_proof.bin");
    const uint8_t ecb_ct32[32] = {0x39, 0x25, 0x84, 0x1d, 0x02, 0xdc, 0x09, 0xfb, 0xdc, 0x11, 0x85, 0x97, 0x19, 0x6a, 0x0b, 0x32,         // FIPS-197 appendix B: what the fixture proves under ECB,
                                  0x39, 0x25, 0x84, 0x1d, 0x02, 0xdc, 0x09, 0xfb, 0xdc, 0x11, 0x85, 0x97, 0x19, 0x6a, 0x0b, 0x32};        // twice (a two-chunk ciphertext)
    const uint8_t fips_pt32[32] = {0x32, 0x43, 0xf6, 0xa8, 0x88, 0x5a, 0x30, 0x8d, 0x31, 0x31, 0x98, 0xa2, 0xe0, 0x37, 0x07, 0x34,
                                   0x32, 0x43, 0xf6, 0xa8, 0x88, 0x5a, 0x30, 0x8d, 0x31, 0x31, 0x98, 0xa2, 0xe0, 0x37, 0x07, 0x34};
    const uint8_t iv[16] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
    uint8_t zero96[96] = {0}, ones4[4] = {0xff, 0xff, 0xff, 0xff};
    zkaes_vk *vk = nullptr, *vk_ark = nullptr, *vk_512 = nullptr;
    CHECK(zkaes_vk_deserialize(vkb.data(), vkb.size(), &vk) == 0 && vk);
    if (!vk) return 1;
    {
        uint8_t *ark = nullptr; size_t ark_len = 0;
        CHECK(zkaes_vk_serialize_ark(vk, &ark, &ark_len) == 0 && ark && ark_len > 32);
        CHECK(zkaes_vk_deserialize_ark(ark, ark_len, &vk_ark) == 0 && vk_ark);
        uint64_t ninst = 0;
        for (int i = 0; i < 8; i++) ninst |= (uint64_t)ark[24 + i] << (8 * i);
        CHECK(ninst == 256);
        ark[25] = 0x02; ark[24] = 0x00;                                                         // |X| = 512: the shape of a 16-byte ECB statement with 16 mask and 128 revealed bits
        CHECK(zkaes_vk_deserialize_ark(ark, ark_len, &vk_512) == 0 && vk_512);
        zkaes_bytes_free(ark);
    }
    if (!vk_ark || !vk_512) return 1;
    int acc = 7, each[2] = {7, 7};
    size_t n_acc = 7, lens[2] = {proof.size(), proof.size()};
    std::vector<uint8_t> two(proof);
    two.insert(two.end(), proof.begin(), proof.end());
    CHECK(zkaes_verify_encryption(vk, proof.data(), proof.size(), ecb_ct32, 16, &acc) == 0 && acc == 1);            // (the fixtures are what they claim to be)
    auto ct16 = exact(ecb_ct32, 16), ct32 = exact(ecb_ct32, 32), ct17 = exact(ecb_ct32, 17), mask2 = exact(ones4, 2), mask4 = exact(ones4, 4), rev16 = exact(fips_pt32, 16), rev32 = exact(fips_pt32, 32),
         zmask = exact(zero96, 4), zrev = exact(zero96, 32), st2 = exact(zero96, 64);
    uint8_t m17[3] = {0xff, 0xff, 0x01};
    for (int shown = 0; shown < 2; shown++) {                                                    // everything revealed (the true plaintext), nothing revealed
        const uint8_t *m2 = shown ? mask2.get() : zmask.get(), *m4 = shown ? mask4.get() : zmask.get(), *r16 = shown ? rev16.get() : zrev.get(), *r32 = shown ? rev32.get() : zrev.get();
        // the stored key knows its 128 public bits: no reveal shape fits, every call is an error and nothing is accepted
        each[0] = each[1] = 7; n_acc = 7;
        CHECK(zkaes_verify_reveal_chunked(vk, ZKAES_CIRCUIT_AES, proof.data(), lens, 1, nullptr, ct16.get(), 16, nullptr, 0, nullptr, m2, 2, r16, each, &n_acc) != 0 && each[0] == 0 && n_acc == 0);
        CHECK(zkaes_verify_reveal_chunked(vk, ZKAES_CIRCUIT_AES, two.data(), lens, 2, nullptr, ct32.get(), 32, nullptr, 0, nullptr, m4, 4, r32, each, &n_acc) != 0 && each[0] == 0 && each[1] == 0 && n_acc == 0);
        CHECK(zkaes_verify_reveal_chunked(vk, ZKAES_CIRCUIT_AES_CBC, proof.data(), lens, 1, iv, ct16.get(), 16, nullptr, 0, nullptr, m2, 2, r16, each, &n_acc) != 0 && n_acc == 0);
        acc = 7;
        CHECK(zkaes_verify_encryption_gcm_reveal(vk, proof.data(), proof.size(), iv, nullptr, 0, ct16.get(), 16, iv, nullptr, 0, nullptr, nullptr, m2, 2, r16, &acc) != 0 && acc == 0);
        // the transported key knows |X| = 256 only, and every reveal shape of 16 bytes has 272 inputs or more: rejected, not an error
        each[0] = each[1] = 7; n_acc = 7;
        CHECK(zkaes_verify_reveal_chunked(vk_ark, ZKAES_CIRCUIT_AES, two.data(), lens, 2, nullptr, ct32.get(), 32, nullptr, 0, nullptr, m4, 4, r32, each, &n_acc) == 0 && each[0] == 0 && each[1] == 0 && n_acc == 0);
        acc = 7;
        CHECK(zkaes_verify_encryption_gcm_reveal(vk_ark, proof.data(), proof.size(), iv, nullptr, 0, ct16.get(), 16, iv, nullptr, 0, nullptr, nullptr, m2, 2, r16, &acc) == 0 && acc == 0);
        // |X| = 512: the 16-byte ECB reveal statement fits, so the proof is parsed and checked -- and fails: it is a proof of a key without reveal
        each[0] = each[1] = 7; n_acc = 7;
        CHECK(zkaes_verify_reveal_chunked(vk_512, ZKAES_CIRCUIT_AES, proof.data(), lens, 1, nullptr, ct16.get(), 16, nullptr, 0, nullptr, m2, 2, r16, each, &n_acc) == 0 && each[0] == 0 && n_acc == 0);
        CHECK(zkaes_verify_reveal_chunked(vk_512, ZKAES_CIRCUIT_AES, two.data(), lens, 2, nullptr, ct32.get(), 32, nullptr, 0, nullptr, m4, 4, r32, each, &n_acc) == 0 && each[0] == 0 && each[1] == 0 && n_acc == 0);
        CHECK(zkaes_verify_reveal_chunked(vk_512, ZKAES_CIRCUIT_AES, two.data(), lens, 2, nullptr, ct32.get(), 32, nullptr, 0, nullptr, m4, 4, r32, nullptr, nullptr) == 0);
        CHECK(zkaes_verify_reveal_chunked(vk_512, ZKAES_CIRCUIT_AES_CBC, proof.data(), lens, 1, iv, ct16.get(), 16, nullptr, 0, nullptr, m2, 2, r16, each, &n_acc) == 0 && each[0] == 0);
        acc = 7;
        CHECK(zkaes_verify_encryption_gcm_reveal(vk_512, proof.data(), proof.size(), iv, nullptr, 0, ct16.get(), 16, iv, nullptr, 0, nullptr, nullptr, m2, 2, r16, &acc) == 0 && acc == 0);
    }
    // arguments that do not go together: errors, whatever the key
    for (zkaes_vk *k : {vk, vk_ark, vk_512}) {
        uint8_t hidden[2] = {0xfe, 0xff}, beyond[3] = {0xff, 0xff, 0x03};
        each[0] = 7; n_acc = 7;
        CHECK(zkaes_verify_reveal_chunked(k, ZKAES_CIRCUIT_AES, proof.data(), lens, 1, nullptr, ct16.get(), 16, nullptr, 0, nullptr, hidden, 2, rev16.get(), each, &n_acc) != 0 && each[0] == 0 && n_acc == 0);      // revealed[0] != 0 under mask bit 0 = 0
        CHECK(zkaes_verify_reveal_chunked(k, ZKAES_CIRCUIT_AES_CTR, proof.data(), lens, 1, iv, ct17.get(), 17, nullptr, 0, nullptr, beyond, 3, zrev.get(), each, &n_acc) != 0 && n_acc == 0);                      // mask bit 17 of a 17-byte message
        CHECK(zkaes_verify_reveal_chunked(k, ZKAES_CIRCUIT_AES_CTR, proof.data(), lens, 1, iv, ct17.get(), 17, nullptr, 0, nullptr, m17, 2, zrev.get(), each, &n_acc) != 0);                                       // a mask of the wrong length
        acc = 7;
        CHECK(zkaes_verify_encryption_gcm_reveal(k, proof.data(), proof.size(), iv, nullptr, 0, ct16.get(), 16, iv, nullptr, 0, nullptr, nullptr, hidden, 2, rev16.get(), &acc) != 0 && acc == 0);
        CHECK(zkaes_verify_encryption_gcm_reveal(k, proof.data(), proof.size(), iv, nullptr, 0, ct17.get(), 17, iv, nullptr, 0, nullptr, nullptr, beyond, 3, zrev.get(), &acc) != 0 && acc == 0);
        CHECK(zkaes_verify_encryption_gcm_reveal(k, proof.data(), proof.size(), iv, nullptr, 0, ct16.get(), 16, iv, nullptr, 0, st2.get(), nullptr, mask2.get(), 2, rev16.get(), &acc) != 0);      // h_in without h_out
        CHECK(zkaes_verify_reveal_chunked(k, ZKAES_CIRCUIT_AES, proof.data(), lens, 1, nullptr, ct16.get(), 16, nullptr, 0, nullptr, nullptr, 2, rev16.get(), each, &n_acc) != 0);
        CHECK(zkaes_verify_reveal_chunked(k, ZKAES_CIRCUIT_AES, proof.data(), lens, 1, nullptr, ct16.get(), 16, nullptr, 0, nullptr, mask2.get(), 2, nullptr, each, &n_acc) != 0);
        CHECK(zkaes_verify_reveal_chunked(k, ZKAES_CIRCUIT_AES_GCM, proof.data(), lens, 1, nullptr, ct16.get(), 16, nullptr, 0, nullptr, mask2.get(), 2, rev16.get(), each, &n_acc) != 0);
        CHECK(zkaes_verify_reveal_chunked(k, ZKAES_CIRCUIT_AES, proof.data(), lens, 1, nullptr, ct16.get(), 16, nullptr, 16, nullptr, mask2.get(), 2, rev16.get(), each, &n_acc) != 0);
        CHECK(zkaes_verify_reveal_chunked(k, ZKAES_CIRCUIT_AES, proof.data(), lens, 0, nullptr, ct16.get(), 16, nullptr, 0, nullptr, mask2.get(), 2, rev16.get(), nullptr, &n_acc) != 0);
        CHECK(zkaes_verify_reveal_chunked(k, ZKAES_CIRCUIT_AES_CTR, two.data(), lens, 2, iv, ct32.get(), 30, nullptr, 0, nullptr, mask4.get(), 4, rev32.get(), each, &n_acc) != 0);      // two ragged CTR chunks
    }
    for (size_t cut = 0; cut < proof.size(); cut++) {                                           // every truncation, in a heap buffer of exactly that size, as chunk 0 of two: chunk 1 is
        const bool whole = cut % 96 == 0;                                                       // the whole proof (parsed and checked) now and then, else one byte that does not parse
        const size_t second = whole ? proof.size() : 1;
        std::vector<uint8_t> t(proof.begin(), proof.begin() + cut);
        t.insert(t.end(), proof.begin(), proof.begin() + second);
        auto buf = exact(t.data(), t.size());
        size_t l2[2] = {cut, second};
        each[0] = each[1] = 7; n_acc = 7;
        CHECK(zkaes_verify_reveal_chunked(vk_512, ZKAES_CIRCUIT_AES, buf.get(), l2, 2, nullptr, ct32.get(), 32, nullptr, 0, nullptr, mask4.get(), 4, rev32.get(), each, &n_acc) == 0 && each[0] == 0 && each[1] == 0 && n_acc == 0);
        auto lone = exact(proof.data(), cut);
        acc = 7;
        CHECK(zkaes_verify_encryption_gcm_reveal(vk_512, lone.get(), cut, iv, nullptr, 0, ct16.get(), 16, iv, nullptr, 0, nullptr, nullptr, mask2.get(), 2, rev16.get(), &acc) != 0 && acc == 0);      // (the lone GCM form reports a proof that does not parse)
    }
    srand(0x4e7);
    for (int round = 0; round < 24; round++) {                                                  // garbage of the proof's length, and the proof with one byte changed
        std::vector<uint8_t> g(proof);
        if (round & 1) for (auto &b : g) b = (uint8_t)rand(); else g[(size_t)rand() % g.size()] ^= (uint8_t)(1 + rand() % 255);
        auto buf = exact(g.data(), g.size());
        each[0] = 7; n_acc = 7;
        CHECK(zkaes_verify_reveal_chunked(vk_512, ZKAES_CIRCUIT_AES, buf.get(), lens, 1, nullptr, ct16.get(), 16, nullptr, 0, nullptr, mask2.get(), 2, rev16.get(), each, &n_acc) == 0 && each[0] == 0 && n_acc == 0);
    }
    zkaes_vk_free(vk);
    zkaes_vk_free(vk_ark);
    zkaes_vk_free(vk_512);
    if (fails) { fprintf(stderr, "reveal_host_check: %d failure(s)\n", fails); return 1; }
    printf("reveal_host_check ok\n");
    return 0;
}
