// tests/keytag_host_check.cpp -- stand-alone check of the host-only key-tag entry points of include/zkaes.h, built by tests/test_keytag_host.py with
// -fsanitize=address,undefined together with csrc/circuit.cpp, csrc/marlin_codec.cpp and csrc/capi_host.cpp (no HIP, no GPU):
//   * zkaes_key_tag for the three FIPS-197 appendix C keys, key and output in heap buffers of exactly their size, equals zkaes_ecb_ciphertext_ks of D_0 || D_1 spelled out
//     here; wrong key lengths, T outside {1, 2} and null arguments are errors;
//   * zkaes_circuit_info_kt at T = 0 equals zkaes_circuit_info_ks, grows by 128 instance variables per tag block, and refuses T = 3 and a tagged ops circuit;
//   * zkaes_verify_chunked_kt and zkaes_verify_encryption_gcm_kt, fed the committed ECB verifying key and proof: the key as stored (it knows its 128 public bits: every
//     tagged shape is an error), after the ark transport (|X| = 256: no tagged shape fits, every chunk is rejected), and the ark image with |X| patched to 512, which the
//     16-byte ECB statement with a 16-byte tag does fit -- there the proof is parsed and checked, whole, truncated at every length and as garbage, one and two chunks: a
//     chunk that does not parse is a rejected chunk, not an error.  Nothing is ever accepted, key_tag_len other than 16 or 32 is an error, and no call touches memory it
//     should not.
// usage: keytag_host_check <directory of the golden fixtures>.  Prints "keytag_host_check ok" and exits 0, or says what went wrong and exits 1.
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
    // ---- the tag: D_t = "zkaes-keyta", t, four zero bytes
    const uint8_t d01[32] = {0x7a, 0x6b, 0x61, 0x65, 0x73, 0x2d, 0x6b, 0x65, 0x79, 0x74, 0x61, 0x00, 0, 0, 0, 0, 0x7a, 0x6b, 0x61, 0x65, 0x73, 0x2d, 0x6b, 0x65, 0x79, 0x74, 0x61, 0x01, 0, 0, 0, 0};
    uint8_t seq[33];
    for (int i = 0; i < 33; i++) seq[i] = (uint8_t)i;
    for (size_t klen : {(size_t)16, (size_t)24, (size_t)32}) {
        auto key = exact(seq, klen);
        uint8_t want[32];
        CHECK(zkaes_ecb_ciphertext_ks(d01, 32, key.get(), klen, want) == 0);
        for (size_t T : {(size_t)1, (size_t)2}) {
            std::unique_ptr<uint8_t[]> out(new uint8_t[16 * T]);
            CHECK(zkaes_key_tag(key.get(), klen, T, out.get()) == 0);
            CHECK(memcmp(out.get(), want, 16 * T) == 0);
        }
        uint8_t out[32];
        CHECK(zkaes_key_tag(key.get(), klen, 0, out) != 0);
        CHECK(zkaes_key_tag(key.get(), klen, 3, out) != 0);
        CHECK(zkaes_key_tag(nullptr, klen, 1, out) != 0);
        CHECK(zkaes_key_tag(key.get(), klen, 1, nullptr) != 0);
    }
    for (size_t klen : {(size_t)0, (size_t)15, (size_t)20, (size_t)33}) {
        auto key = exact(seq, klen);
        uint8_t out[32];
        CHECK(zkaes_key_tag(key.get(), klen, 1, out) != 0);
    }
    // ---- circuit queries
    {
        uint64_t a[12], b[12];
        CHECK(zkaes_circuit_info_ks(ZKAES_CIRCUIT_AES, 128, 16, 0, a) == 0 && zkaes_circuit_info_kt(ZKAES_CIRCUIT_AES, 128, 0, 16, 0, b) == 0 && memcmp(a, b, sizeof a) == 0);
        CHECK(zkaes_circuit_info_kt(ZKAES_CIRCUIT_AES, 128, 1, 16, 0, b) == 0 && b[1] == a[1] + 128);
        CHECK(zkaes_circuit_info_kt(ZKAES_CIRCUIT_AES, 128, 2, 16, 0, b) == 0 && b[1] == a[1] + 256);
        CHECK(zkaes_circuit_info_kt(ZKAES_CIRCUIT_AES, 128, 3, 16, 0, b) != 0);
        CHECK(zkaes_circuit_info_kt(ZKAES_CIRCUIT_OPS_XOR, 128, 1, 0, 0, b) != 0);
        uint64_t rows = 0, nnz = 0;
        CHECK(zkaes_circuit_matrix_kt(ZKAES_CIRCUIT_AES, 128, 3, 16, 0, 0, &rows, &nnz, nullptr, nullptr, nullptr) != 0);
    }
    // ---- the ECB fixtures through the tagged verifiers
    const std::vector<uint8_t> vkb = slurp(gold + "/gpu_aes16_vk.bin"), proof = slurp(gold + "/gpu_aes16_proof.bin");
    const uint8_t ecb_ct32[32] = {0x39, 0x25, 0x84, 0x1d, 0x02, 0xdc, 0x09, 0xfb, 0xdc, 0x11, 0x85, 0x97, 0x19, 0x6a, 0x0b, 0x32,         // FIPS-197 appendix B: what the fixture proves under ECB,
                                  0x39, 0x25, 0x84, 0x1d, 0x02, 0xdc, 0x09, 0xfb, 0xdc, 0x11, 0x85, 0x97, 0x19, 0x6a, 0x0b, 0x32};        // twice (a two-chunk ciphertext)
    const uint8_t iv[16] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16}, zero32[32] = {0};
    zkaes_vk *vk = nullptr, *vk_ark = nullptr, *vk_512 = nullptr;
    CHECK(zkaes_vk_deserialize(vkb.data(), vkb.size(), &vk) == 0 && vk);
    if (!vk) return 1;
    {
        uint8_t *ark = nullptr; size_t ark_len = 0;
        CHECK(zkaes_vk_serialize_ark(vk, &ark, &ark_len) == 0 && ark && ark_len > 32);
        CHECK(zkaes_vk_deserialize_ark(ark, ark_len, &vk_ark) == 0 && vk_ark);
        uint64_t ninst = 0;
        for (int i = 0; i < 8; i++) ninst |= (uint64_t)ark[24 + i] << (8 * i);
        CHECK(ninst == 256);                                                                    // index info: variables, constraints, non-zeros, instance variables
        ark[25] = 0x02; ark[24] = 0x00;                                                         // |X| = 512: the shape of a 16-byte ECB statement with one tag block
        CHECK(zkaes_vk_deserialize_ark(ark, ark_len, &vk_512) == 0 && vk_512);
        zkaes_bytes_free(ark);
    }
    if (!vk_ark || !vk_512) return 1;
    int acc = 7, each[2] = {7, 7};
    size_t n_acc = 7, lens[2] = {proof.size(), proof.size()};
    std::vector<uint8_t> two(proof);
    two.insert(two.end(), proof.begin(), proof.end());
    CHECK(zkaes_verify_encryption(vk, proof.data(), proof.size(), ecb_ct32, 16, &acc) == 0 && acc == 1);            // (the fixtures are what they claim to be)
    auto tag16 = exact(zero32, 16), tag32 = exact(zero32, 32), ct16 = exact(ecb_ct32, 16), ct32 = exact(ecb_ct32, 32), ct17 = exact(ecb_ct32, 17);
    // the stored key knows its 128 public bits: with 128 or 256 tag bits behind them no shape fits, every call is an error and nothing is accepted
    for (size_t tl : {(size_t)16, (size_t)32}) {
        const uint8_t *tg = tl == 16 ? tag16.get() : tag32.get();
        each[0] = each[1] = 7; n_acc = 7;
        CHECK(zkaes_verify_chunked_kt(vk, ZKAES_CIRCUIT_AES, proof.data(), lens, 1, nullptr, ct16.get(), 16, tg, tl, each, &n_acc) != 0 && each[0] == 0 && n_acc == 0);
        CHECK(zkaes_verify_chunked_kt(vk, ZKAES_CIRCUIT_AES, two.data(), lens, 2, nullptr, ct32.get(), 32, tg, tl, each, &n_acc) != 0 && each[0] == 0 && each[1] == 0 && n_acc == 0);
        CHECK(zkaes_verify_chunked_kt(vk, ZKAES_CIRCUIT_AES_CBC, proof.data(), lens, 1, iv, ct16.get(), 16, tg, tl, each, &n_acc) != 0 && n_acc == 0);
        CHECK(zkaes_verify_chunked_kt(vk, ZKAES_CIRCUIT_AES_CTR, proof.data(), lens, 1, iv, ct17.get(), 17, tg, tl, each, &n_acc) != 0 && n_acc == 0);
        acc = 7;
        CHECK(zkaes_verify_encryption_gcm_kt(vk, proof.data(), proof.size(), iv, nullptr, 0, ct17.get(), 17, iv, tg, tl, &acc) != 0 && acc == 0);
        // the transported key knows |X| = 256 only, and every tagged shape has more than 255 inputs: rejected, not an error
        each[0] = each[1] = 7; n_acc = 7;
        CHECK(zkaes_verify_chunked_kt(vk_ark, ZKAES_CIRCUIT_AES, two.data(), lens, 2, nullptr, ct32.get(), 32, tg, tl, each, &n_acc) == 0 && each[0] == 0 && each[1] == 0 && n_acc == 0);
        CHECK(zkaes_verify_chunked_kt(vk_ark, ZKAES_CIRCUIT_AES_CTR, proof.data(), lens, 1, iv, ct17.get(), 17, tg, tl, each, &n_acc) == 0 && each[0] == 0 && n_acc == 0);
        acc = 7;
        CHECK(zkaes_verify_encryption_gcm_kt(vk_ark, proof.data(), proof.size(), iv, nullptr, 0, ct17.get(), 1, iv, tg, tl, &acc) == 0 && acc == 0);
    }
    // key_tag_len other than 16 or 32, kinds and iv arguments that do not go together, shapes that are no chunks: errors, whatever the key
    for (zkaes_vk *k : {vk, vk_ark, vk_512}) {
        for (size_t tl : {(size_t)0, (size_t)15, (size_t)17, (size_t)31, (size_t)48}) {
            auto tg = exact(zero32, tl > 32 ? 32 : tl);
            CHECK(zkaes_verify_chunked_kt(k, ZKAES_CIRCUIT_AES, proof.data(), lens, 1, nullptr, ct16.get(), 16, tg.get(), tl, each, &n_acc) != 0 && n_acc == 0);
            acc = 7;
            CHECK(zkaes_verify_encryption_gcm_kt(k, proof.data(), proof.size(), iv, nullptr, 0, ct16.get(), 16, iv, tg.get(), tl, &acc) != 0 && acc == 0);
        }
        CHECK(zkaes_verify_chunked_kt(k, ZKAES_CIRCUIT_AES_GCM, proof.data(), lens, 1, nullptr, ct16.get(), 16, tag16.get(), 16, each, &n_acc) != 0);
        CHECK(zkaes_verify_chunked_kt(k, ZKAES_CIRCUIT_OPS_XOR, proof.data(), lens, 1, nullptr, ct16.get(), 16, tag16.get(), 16, each, &n_acc) != 0);
        CHECK(zkaes_verify_chunked_kt(k, ZKAES_CIRCUIT_AES, proof.data(), lens, 1, iv, ct16.get(), 16, tag16.get(), 16, each, &n_acc) != 0);
        CHECK(zkaes_verify_chunked_kt(k, ZKAES_CIRCUIT_AES_CBC, proof.data(), lens, 1, nullptr, ct16.get(), 16, tag16.get(), 16, each, &n_acc) != 0);
        CHECK(zkaes_verify_chunked_kt(k, ZKAES_CIRCUIT_AES, proof.data(), lens, 0, nullptr, ct16.get(), 16, tag16.get(), 16, nullptr, &n_acc) != 0);
        CHECK(zkaes_verify_chunked_kt(k, ZKAES_CIRCUIT_AES, proof.data(), lens, 1, nullptr, ct16.get(), 0, tag16.get(), 16, each, &n_acc) != 0);
        CHECK(zkaes_verify_chunked_kt(k, ZKAES_CIRCUIT_AES, proof.data(), lens, 1, nullptr, ct17.get(), 17, tag16.get(), 16, each, &n_acc) != 0);
        CHECK(zkaes_verify_chunked_kt(k, ZKAES_CIRCUIT_AES_CTR, two.data(), lens, 2, iv, ct32.get(), 30, tag16.get(), 16, each, &n_acc) != 0);      // two ragged CTR chunks
        CHECK(zkaes_verify_chunked_kt(k, ZKAES_CIRCUIT_AES, proof.data(), lens, 1, nullptr, ct16.get(), 16, nullptr, 16, each, &n_acc) != 0);
        CHECK(zkaes_verify_chunked_kt(k, ZKAES_CIRCUIT_AES, nullptr, lens, 1, nullptr, ct16.get(), 16, tag16.get(), 16, each, &n_acc) != 0);
        CHECK(zkaes_verify_encryption_gcm_kt(k, proof.data(), proof.size(), iv, nullptr, 0, ct16.get(), 0, iv, tag16.get(), 16, &acc) != 0);
        CHECK(zkaes_verify_encryption_gcm_kt(k, proof.data(), proof.size(), iv, nullptr, 0, ct16.get(), 16, iv, nullptr, 16, &acc) != 0);
    }
    // |X| = 512: the 16-byte ECB statement with a 16-byte tag fits, so the proof is parsed and checked -- and fails; a 32-byte tag pads to the same |X| and fails too
    each[0] = each[1] = 7; n_acc = 7;
    CHECK(zkaes_verify_chunked_kt(vk_512, ZKAES_CIRCUIT_AES, proof.data(), lens, 1, nullptr, ct16.get(), 16, tag16.get(), 16, each, &n_acc) == 0 && each[0] == 0 && n_acc == 0);
    CHECK(zkaes_verify_chunked_kt(vk_512, ZKAES_CIRCUIT_AES, two.data(), lens, 2, nullptr, ct32.get(), 32, tag16.get(), 16, each, &n_acc) == 0 && each[0] == 0 && each[1] == 0 && n_acc == 0);
    CHECK(zkaes_verify_chunked_kt(vk_512, ZKAES_CIRCUIT_AES, two.data(), lens, 2, nullptr, ct32.get(), 32, tag16.get(), 16, nullptr, nullptr) == 0);
    CHECK(zkaes_verify_chunked_kt(vk_512, ZKAES_CIRCUIT_AES, proof.data(), lens, 1, nullptr, ct16.get(), 16, tag32.get(), 32, each, &n_acc) == 0 && each[0] == 0 && n_acc == 0);
    CHECK(zkaes_verify_chunked_kt(vk_512, ZKAES_CIRCUIT_AES_CBC, proof.data(), lens, 1, iv, ct16.get(), 16, tag16.get(), 16, each, &n_acc) == 0 && each[0] == 0);      // 128 + 128 + 128 inputs
    CHECK(zkaes_verify_chunked_kt(vk_512, ZKAES_CIRCUIT_AES_CTR, proof.data(), lens, 1, iv, ct17.get(), 17, tag16.get(), 16, each, &n_acc) == 0 && each[0] == 0);      // ragged lone CTR
    acc = 7;
    CHECK(zkaes_verify_encryption_gcm_kt(vk_512, proof.data(), proof.size(), iv, nullptr, 0, ct16.get(), 1, iv, tag16.get(), 16, &acc) == 0 && acc == 0);               // 224 + 8 + 128 inputs
    for (size_t cut = 0; cut < proof.size(); cut++) {                                           // every truncation, in a heap buffer of exactly that size, as chunk 0 of two: chunk 1 is
        const bool whole = cut % 96 == 0;                                                       // the whole proof (parsed and checked) now and then, else one byte that does not parse
        const size_t second = whole ? proof.size() : 1;
        std::vector<uint8_t> t(proof.begin(), proof.begin() + cut);
        t.insert(t.end(), proof.begin(), proof.begin() + second);
        auto buf = exact(t.data(), t.size());
        size_t l2[2] = {cut, second};
        each[0] = each[1] = 7; n_acc = 7;
        CHECK(zkaes_verify_chunked_kt(vk_512, ZKAES_CIRCUIT_AES, buf.get(), l2, 2, nullptr, ct32.get(), 32, tag16.get(), 16, each, &n_acc) == 0 && each[0] == 0 && each[1] == 0 && n_acc == 0);
        auto lone = exact(proof.data(), cut);
        acc = 7;
        CHECK(zkaes_verify_encryption_gcm_kt(vk_512, lone.get(), cut, iv, nullptr, 0, ct16.get(), 1, iv, tag16.get(), 16, &acc) != 0 && acc == 0);      // (the lone GCM form reports a proof that does not parse)
    }
    srand(0x7a6);
    for (int round = 0; round < 24; round++) {                                                  // garbage of the proof's length, and the proof with one byte changed
        std::vector<uint8_t> g(proof);
        if (round & 1) for (auto &b : g) b = (uint8_t)rand(); else g[(size_t)rand() % g.size()] ^= (uint8_t)(1 + rand() % 255);
        auto buf = exact(g.data(), g.size());
        each[0] = 7; n_acc = 7;
        CHECK(zkaes_verify_chunked_kt(vk_512, ZKAES_CIRCUIT_AES, buf.get(), lens, 1, nullptr, ct16.get(), 16, tag16.get(), 16, each, &n_acc) == 0 && each[0] == 0 && n_acc == 0);
    }
    zkaes_vk_free(vk);
    zkaes_vk_free(vk_ark);
    zkaes_vk_free(vk_512);
    if (fails) { fprintf(stderr, "keytag_host_check: %d failure(s)\n", fails); return 1; }
    printf("keytag_host_check ok\n");
    return 0;
}
