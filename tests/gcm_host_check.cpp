// tests/gcm_host_check.cpp -- stand-alone check of the host-only GCM entry points of include/zkaes.h, built by tests/test_gcm_host.py with
// -fsanitize=address,undefined together with csrc/circuit.cpp, csrc/marlin_codec.cpp and csrc/capi_host.cpp (no HIP, no GPU):
//   * zkaes_gcm_encrypt reproduces McGrew-Viega test cases 1-4 (AES-128) into heap buffers of exactly the message's size, with aad buffers of exactly the aad's size, so
//     a read past L or A is a sanitizer report; prefixes of test case 4 with cut aad go through encrypt and decrypt and come back;
//   * zkaes_gcm_decrypt gives the plaintext back, and after one flipped bit of the tag, the ciphertext or the aad reports ok = 0 and leaves the output buffer untouched;
//   * zkaes_verify_encryption_gcm, fed the committed ECB verifying key and proof -- whole, the proof truncated at every length, the key as stored and after the ark
//     transport (which keeps only the padded input count) -- never accepts and never touches memory it should not; null arguments and an empty ciphertext are errors.
// usage: gcm_host_check <directory of the golden fixtures>.  Prints "gcm_host_check ok" and exits 0, or says what went wrong and exits 1.
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
static std::vector<uint8_t> unhex(const char *h) {
    std::vector<uint8_t> v;
    for (size_t i = 0; h[i] && h[i + 1]; i += 2) { unsigned x; sscanf(h + i, "%2x", &x); v.push_back((uint8_t)x); }
    return v;
}
// a heap copy of exactly n bytes (nullptr for n = 0): the sanitizer watches both ends
static std::unique_ptr<uint8_t[]> exact(const uint8_t *src, size_t n) {
    std::unique_ptr<uint8_t[]> p(n ? new uint8_t[n] : nullptr);
    if (n) memcpy(p.get(), src, n);
    return p;
}

static void roundtrip(const std::vector<uint8_t> &key, const std::vector<uint8_t> &iv, const uint8_t *pt, size_t L, const uint8_t *aad, size_t A, const uint8_t *want_ct, const uint8_t *want_tag) {
    auto m = exact(pt, L), a = exact(aad, A);
    std::unique_ptr<uint8_t[]> ct(L ? new uint8_t[L] : nullptr), back(L ? new uint8_t[L] : nullptr);
    uint8_t tag[16];
    int ok = 7;
    CHECK(zkaes_gcm_encrypt(m.get(), L, key.data(), iv.data(), a.get(), A, ct.get(), tag) == 0);
    if (want_ct) CHECK(L == 0 || memcmp(ct.get(), want_ct, L) == 0);
    if (want_tag) CHECK(memcmp(tag, want_tag, 16) == 0);
    CHECK(zkaes_gcm_decrypt(ct.get(), L, key.data(), iv.data(), a.get(), A, tag, back.get(), &ok) == 0 && ok == 1);
    CHECK(L == 0 || memcmp(back.get(), pt, L) == 0);
    // one flipped bit of the tag, of the ciphertext, of the aad: ok = 0 and the output buffer keeps what it held
    for (int what = 0; what < 3; what++) {
        if ((what == 1 && L == 0) || (what == 2 && A == 0)) continue;
        auto c2 = exact(ct.get(), L), a2 = exact(aad, A);
        uint8_t t2[16];
        memcpy(t2, tag, 16);
        if (what == 0) t2[15] ^= 0x01;
        if (what == 1) c2[L - 1] ^= 0x80;
        if (what == 2) a2[A - 1] ^= 0x10;
        if (L) memset(back.get(), 0xEE, L);
        ok = 7;
        CHECK(zkaes_gcm_decrypt(c2.get(), L, key.data(), iv.data(), a2.get(), A, t2, back.get(), &ok) == 0 && ok == 0);
        for (size_t i = 0; i < L; i++) CHECK(back[i] == 0xEE);
    }
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s <golden dir>\n", argv[0]); return 1; }
    const std::string gold = argv[1];
    // ---- McGrew-Viega, "The Galois/Counter Mode of Operation", appendix B, test cases 1-4
    const std::vector<uint8_t> k0(16, 0), iv0(12, 0), z16(16, 0);
    const std::vector<uint8_t> k3 = unhex("feffe9928665731c6d6a8f9467308308"), iv3 = unhex("cafebabefacedbaddecaf888");
    const std::vector<uint8_t> p3 = unhex("d9313225f88406e5a55909c5aff5269a86a7a9531534f7da2e4c303d8a318a721c3c0c95956809532fcf0e2449a6b525b16aedf5aa0de657ba637b391aafd255");
    const std::vector<uint8_t> c3 = unhex("42831ec2217774244b7221b784d0d49ce3aa212f2c02a4e035c17e2329aca12e21d514b25466931c7d8f6a5aac84aa051ba30b396a0aac973d58e091473f5985");
    const std::vector<uint8_t> a4 = unhex("feedfacedeadbeeffeedfacedeadbeefabaddad2");
    roundtrip(k0, iv0, nullptr, 0, nullptr, 0, nullptr, unhex("58e2fccefa7e3061367f1d57a4e7455a").data());
    roundtrip(k0, iv0, z16.data(), 16, nullptr, 0, unhex("0388dace60b6a392f328c2b971b2fe78").data(), unhex("ab6e47d42cec13bdf53a67b21257bddf").data());
    roundtrip(k3, iv3, p3.data(), 64, nullptr, 0, c3.data(), unhex("4d5c2af327cd64a62cf35abd2ba6fab4").data());
    roundtrip(k3, iv3, p3.data(), 60, a4.data(), 20, c3.data(), unhex("5bc94fbc3221a5db94fae95ae7121a47").data());
    for (size_t L : {(size_t)0, (size_t)1, (size_t)15, (size_t)16, (size_t)17, (size_t)33})
        for (size_t A : {(size_t)0, (size_t)5, (size_t)16, (size_t)20}) roundtrip(k3, iv3, p3.data(), L, a4.data(), A, c3.data(), nullptr);       // (the keystream does not depend on the aad)
    {
        uint8_t ct[16], tag[16], msg[16];
        int ok = 7;
        CHECK(zkaes_gcm_encrypt(z16.data(), 16, nullptr, iv0.data(), nullptr, 0, ct, tag) != 0);
        CHECK(zkaes_gcm_encrypt(z16.data(), 16, k0.data(), nullptr, nullptr, 0, ct, tag) != 0);
        CHECK(zkaes_gcm_encrypt(nullptr, 16, k0.data(), iv0.data(), nullptr, 0, ct, tag) != 0);
        CHECK(zkaes_gcm_encrypt(z16.data(), 16, k0.data(), iv0.data(), nullptr, 4, ct, tag) != 0);
        CHECK(zkaes_gcm_encrypt(z16.data(), 16, k0.data(), iv0.data(), nullptr, 0, ct, nullptr) != 0);
        CHECK(zkaes_gcm_decrypt(ct, 16, k0.data(), iv0.data(), nullptr, 0, nullptr, msg, &ok) != 0);
        CHECK(zkaes_gcm_decrypt(ct, 16, k0.data(), iv0.data(), nullptr, 0, tag, msg, nullptr) != 0);
    }
    // ---- the ECB fixtures through the GCM verifier
    const std::vector<uint8_t> vkb = slurp(gold + "/gpu_aes16_vk.bin"), proof = slurp(gold + "/gpu_aes16_proof.bin");
    const std::vector<uint8_t> ecb_ct = unhex("3925841d02dc09fbdc118597196a0b32");          // FIPS-197 appendix B: what the fixture proves under ECB
    const std::vector<uint8_t> tag = unhex("4d5c2af327cd64a62cf35abd2ba6fab4");
    zkaes_vk *vk = nullptr, *vk_ark = nullptr;
    CHECK(zkaes_vk_deserialize(vkb.data(), vkb.size(), &vk) == 0 && vk);
    if (!vk) return 1;
    {
        uint8_t *ark = nullptr; size_t ark_len = 0;
        CHECK(zkaes_vk_serialize_ark(vk, &ark, &ark_len) == 0 && ark);
        CHECK(zkaes_vk_deserialize_ark(ark, ark_len, &vk_ark) == 0 && vk_ark);
        zkaes_bytes_free(ark);
    }
    if (!vk_ark) return 1;
    int acc = 7;
    CHECK(zkaes_verify_encryption(vk, proof.data(), proof.size(), ecb_ct.data(), 16, &acc) == 0 && acc == 1);      // (the fixtures are what they claim to be)
    // the stored key knows its statement has 128 public bits: no GCM shape has as few (224 at the least), so every shape is an error and nothing is accepted
    for (size_t L : {(size_t)0, (size_t)1, (size_t)16, (size_t)17, (size_t)64})
        for (size_t A : {(size_t)0, (size_t)5, (size_t)20}) {
            auto c = exact(c3.data(), L), a = exact(a4.data(), A);
            uint8_t dummy = 0;
            acc = 7;
            CHECK(zkaes_verify_encryption_gcm(vk, proof.data(), proof.size(), iv3.data(), a.get(), A, L ? c.get() : &dummy, L, tag.data(), &acc) != 0 && acc == 0);
        }
    // the transported key knows |X| = 256 only: 224 + 8 (A + L) inputs pad to 256 for A + L <= 3 and fail the proof's checks; other sums are another |X|, also rejected
    for (size_t L : {(size_t)1, (size_t)3, (size_t)16, (size_t)64})
        for (size_t A : {(size_t)0, (size_t)2, (size_t)20}) {
            auto c = exact(c3.data(), L), a = exact(a4.data(), A);
            acc = 7;
            CHECK(zkaes_verify_encryption_gcm(vk_ark, proof.data(), proof.size(), iv3.data(), a.get(), A, c.get(), L, tag.data(), &acc) == 0 && acc == 0);
        }
    acc = 7;
    CHECK(zkaes_verify_encryption_gcm(vk_ark, proof.data(), proof.size(), iv3.data(), nullptr, 0, ecb_ct.data(), 0, tag.data(), &acc) != 0 && acc == 0);        // L = 0
    CHECK(zkaes_verify_encryption_gcm(vk_ark, proof.data(), proof.size(), nullptr, nullptr, 0, ecb_ct.data(), 1, tag.data(), &acc) != 0);
    CHECK(zkaes_verify_encryption_gcm(vk_ark, proof.data(), proof.size(), iv3.data(), nullptr, 3, ecb_ct.data(), 1, tag.data(), &acc) != 0);
    CHECK(zkaes_verify_encryption_gcm(vk_ark, proof.data(), proof.size(), iv3.data(), nullptr, 0, ecb_ct.data(), 1, nullptr, &acc) != 0);
    for (size_t cut = 0; cut < proof.size(); cut++) {                                           // every truncation, in a heap buffer of exactly that size
        std::vector<uint8_t> t(proof.begin(), proof.begin() + cut);
        if (t.empty()) t.reserve(1);
        acc = 7;
        int rc = zkaes_verify_encryption_gcm(vk_ark, t.data() ? t.data() : proof.data(), cut, iv3.data(), nullptr, 0, ecb_ct.data(), 2, tag.data(), &acc);
        CHECK(rc != 0 && acc == 0);
    }
    zkaes_vk_free(vk);
    zkaes_vk_free(vk_ark);
    if (fails) { fprintf(stderr, "gcm_host_check: %d failure(s)\n", fails); return 1; }
    printf("gcm_host_check ok\n");
    return 0;
}
