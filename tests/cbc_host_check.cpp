// tests/cbc_host_check.cpp -- stand-alone check of the host-only CBC entry points of include/zkaes.h, built by tests/test_cbc_host.py with
// -fsanitize=address,undefined together with csrc/circuit.cpp, csrc/marlin_codec.cpp and csrc/capi_host.cpp (no HIP, no GPU):
//   * zkaes_cbc_ciphertext reproduces NIST SP 800-38A F.2.1 (CBC-AES128.Encrypt), block by block and as one message, and refuses lengths 0 and 17;
//   * zkaes_verify_encryption_cbc and zkaes_verify_cbc_chunked, fed the committed ECB verifying key and proof -- whole, and the proof truncated at every
//     length -- never accept and never touch memory they should not; bad ciphertext lengths are errors.
// usage: cbc_host_check <directory of the golden fixtures>.  Prints "cbc_host_check ok" and exits 0, or says what went wrong and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s <golden dir>\n", argv[0]); return 1; }
    const std::string gold = argv[1];
    // ---- SP 800-38A F.2.1
    const std::vector<uint8_t> key = unhex("2b7e151628aed2a6abf7158809cf4f3c"), iv = unhex("000102030405060708090a0b0c0d0e0f");
    const std::vector<uint8_t> pt = unhex("6bc1bee22e409f96e93d7e117393172aae2d8a571e03ac9c9eb76fac45af8e5130c81c46a35ce411e5fbc1191a0a52eff69f2445df4f9b17ad2b417be66c3710");
    const std::vector<uint8_t> want = unhex("7649abac8119b246cee98e9b12e9197d5086cb9b507219ee95db113a917678b273bed6b8e3c1743b7116e69e222295163ff1caa1681fac09120eca307586e1a7");
    {
        std::vector<uint8_t> ct(64);
        CHECK(zkaes_cbc_ciphertext(pt.data(), 64, key.data(), iv.data(), ct.data()) == 0);
        CHECK(ct == want);
        for (int b = 0; b < 4; b++) {            // block by block, each under the chaining value entering it: what a job split over several calls does
            std::vector<uint8_t> one(16);
            CHECK(zkaes_cbc_ciphertext(pt.data() + 16 * b, 16, key.data(), b ? want.data() + 16 * (b - 1) : iv.data(), one.data()) == 0);
            CHECK(memcmp(one.data(), want.data() + 16 * b, 16) == 0);
        }
        std::vector<uint8_t> tight(16);           // exactly the bytes asked for are written (the sanitizer watches the end of the buffer)
        CHECK(zkaes_cbc_ciphertext(pt.data(), 16, key.data(), iv.data(), tight.data()) == 0);
        CHECK(zkaes_cbc_ciphertext(pt.data(), 0, key.data(), iv.data(), tight.data()) != 0);
        CHECK(zkaes_cbc_ciphertext(pt.data(), 17, key.data(), iv.data(), ct.data()) != 0);
        CHECK(zkaes_cbc_ciphertext(nullptr, 16, key.data(), iv.data(), ct.data()) != 0);
    }
    // ---- the ECB fixtures through the CBC verifiers
    const std::vector<uint8_t> vkb = slurp(gold + "/gpu_aes16_vk.bin"), proof = slurp(gold + "/gpu_aes16_proof.bin");
    const std::vector<uint8_t> ecb_ct = unhex("3925841d02dc09fbdc118597196a0b32");          // FIPS-197 appendix B: what the fixture proves under ECB
    zkaes_vk *vk = nullptr;
    CHECK(zkaes_vk_deserialize(vkb.data(), vkb.size(), &vk) == 0 && vk);
    if (!vk) return 1;
    for (size_t cut : {vkb.size() - 1, vkb.size() / 2, (size_t)12, (size_t)3}) {              // a truncated key never becomes a key
        zkaes_vk *bad = nullptr;
        CHECK(zkaes_vk_deserialize(vkb.data(), cut, &bad) != 0 && !bad);
    }
    int acc = 7;
    CHECK(zkaes_verify_encryption(vk, proof.data(), proof.size(), ecb_ct.data(), 16, &acc) == 0 && acc == 1);      // (the fixtures are what they claim to be)
    acc = 7;
    CHECK(zkaes_verify_encryption_cbc(vk, proof.data(), proof.size(), iv.data(), ecb_ct.data(), 16, &acc) == 0 && acc == 0);
    CHECK(zkaes_verify_encryption_cbc(vk, proof.data(), proof.size(), iv.data(), want.data(), 64, &acc) == 0 && acc == 0);
    for (size_t bad_len : {(size_t)0, (size_t)15, (size_t)17}) {
        acc = 7;
        CHECK(zkaes_verify_encryption_cbc(vk, proof.data(), proof.size(), iv.data(), want.data(), bad_len, &acc) != 0 && acc != 1);
    }
    {
        size_t lens[2] = {proof.size(), proof.size()}, n_ok = 9;
        int each[2] = {7, 7};
        std::vector<uint8_t> two(proof);
        two.insert(two.end(), proof.begin(), proof.end());
        CHECK(zkaes_verify_cbc_chunked(vk, two.data(), lens, 2, iv.data(), want.data(), 32, each, &n_ok) == 0 && n_ok == 0 && each[0] == 0 && each[1] == 0);
        CHECK(zkaes_verify_cbc_chunked(vk, two.data(), lens, 1, iv.data(), ecb_ct.data(), 16, nullptr, nullptr) == 0);
        n_ok = 9;
        CHECK(zkaes_verify_cbc_chunked(vk, two.data(), lens, 2, iv.data(), want.data(), 48, each, &n_ok) != 0 && n_ok == 0);     // 48 bytes are not 2 x whole blocks
        CHECK(zkaes_verify_cbc_chunked(vk, two.data(), lens, 0, iv.data(), want.data(), 32, each, &n_ok) != 0);
        CHECK(zkaes_verify_cbc_chunked(vk, two.data(), lens, 2, iv.data(), want.data(), 0, each, &n_ok) != 0);
    }
    for (size_t cut = 0; cut < proof.size(); cut++) {                                           // every truncation, in a heap buffer of exactly that size
        std::vector<uint8_t> t(proof.begin(), proof.begin() + cut);
        if (t.empty()) t.reserve(1);
        acc = 7;
        int rc = zkaes_verify_encryption_cbc(vk, t.data() ? t.data() : proof.data(), cut, iv.data(), ecb_ct.data(), 16, &acc);
        CHECK(rc != 0 && acc == 0);
        size_t lens[1] = {cut}, n_ok = 9;
        int each[1] = {7};
        rc = zkaes_verify_cbc_chunked(vk, t.data() ? t.data() : proof.data(), lens, 1, iv.data(), ecb_ct.data(), 16, each, &n_ok);
        CHECK(rc == 0 && n_ok == 0 && each[0] == 0);                                            // an unparsable chunk is a rejected chunk
    }
    zkaes_vk_free(vk);
    if (fails) { fprintf(stderr, "cbc_host_check: %d failure(s)\n", fails); return 1; }
    printf("cbc_host_check ok\n");
    return 0;
}
