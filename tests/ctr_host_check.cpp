// tests/ctr_host_check.cpp -- stand-alone check of the host-only CTR entry points of include/zkaes.h, built by tests/test_ctr_host.py with
// -fsanitize=address,undefined together with csrc/circuit.cpp, csrc/marlin_codec.cpp and csrc/capi_host.cpp (no HIP, no GPU):
//   * zkaes_ctr_crypt reproduces NIST SP 800-38A F.5.1 (CTR-AES128.Encrypt) whole and at the prefixes 1, 15, 17 and 33, into heap buffers of exactly that size, is its
//     own inverse, and refuses length 0 and null arguments;
//   * zkaes_ctr_counter_add carries through all 16 bytes, wraps mod 2^128 and may write over its input;
//   * zkaes_verify_encryption_ctr and zkaes_verify_ctr_chunked, fed the committed ECB verifying key and proof -- whole, the proof truncated at every length, the key
//     both as stored and after the ark transport (which keeps only the padded input count) -- never accept and never touch memory they should not.
// usage: ctr_host_check <directory of the golden fixtures>.  Prints "ctr_host_check ok" and exits 0, or says what went wrong and exits 1.
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
    // ---- SP 800-38A F.5.1
    const std::vector<uint8_t> key = unhex("2b7e151628aed2a6abf7158809cf4f3c"), icb = unhex("f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff");
    const std::vector<uint8_t> pt = unhex("6bc1bee22e409f96e93d7e117393172aae2d8a571e03ac9c9eb76fac45af8e5130c81c46a35ce411e5fbc1191a0a52eff69f2445df4f9b17ad2b417be66c3710");
    const std::vector<uint8_t> want = unhex("874d6191b620e3261bef6864990db6ce9806f66b7970fdff8617187bb9fffdff5ae4df3edbd5d35e5b4f09020db03eab1e031dda2fbe03d1792170a0f3009cee");
    for (size_t n : {(size_t)64, (size_t)1, (size_t)15, (size_t)16, (size_t)17, (size_t)33}) {
        std::vector<uint8_t> in(pt.begin(), pt.begin() + n), ct(n), back(n);          // exactly n bytes each: the sanitizer watches both ends
        CHECK(zkaes_ctr_crypt(in.data(), n, key.data(), icb.data(), ct.data()) == 0);
        CHECK(memcmp(ct.data(), want.data(), n) == 0);
        CHECK(zkaes_ctr_crypt(ct.data(), n, key.data(), icb.data(), back.data()) == 0);
        CHECK(back == in);
    }
    {
        std::vector<uint8_t> ct(64), c2(16);
        CHECK(zkaes_ctr_crypt(pt.data(), 0, key.data(), icb.data(), ct.data()) != 0);
        CHECK(zkaes_ctr_crypt(nullptr, 16, key.data(), icb.data(), ct.data()) != 0);
        CHECK(zkaes_ctr_crypt(pt.data(), 16, key.data(), nullptr, ct.data()) != 0);
        // a job split over two calls: the second call's counter comes from zkaes_ctr_counter_add
        uint8_t adv[16];
        CHECK(zkaes_ctr_counter_add(icb.data(), 3, adv) == 0);
        CHECK(zkaes_ctr_crypt(pt.data() + 48, 16, key.data(), adv, c2.data()) == 0);
        CHECK(memcmp(c2.data(), want.data() + 48, 16) == 0);
    }
    {
        uint8_t c[16], out[16], zero[16] = {0};
        memset(c, 0xff, 16);
        CHECK(zkaes_ctr_counter_add(c, 1, out) == 0 && memcmp(out, zero, 16) == 0);                      // wraps mod 2^128
        CHECK(zkaes_ctr_counter_add(c, 0, out) == 0 && memcmp(out, c, 16) == 0);
        memset(c, 0, 16); memset(c + 12, 0xff, 4);
        CHECK(zkaes_ctr_counter_add(c, 1, c) == 0);                                                        // in place; the carry reaches byte 11
        const std::vector<uint8_t> w = unhex("00000000000000000000000100000000");
        CHECK(memcmp(c, w.data(), 16) == 0);
        memset(c, 0, 16);
        CHECK(zkaes_ctr_counter_add(c, 0xffffffffffffffffull, out) == 0);
        const std::vector<uint8_t> w2 = unhex("0000000000000000ffffffffffffffff");
        CHECK(memcmp(out, w2.data(), 16) == 0);
        CHECK(zkaes_ctr_counter_add(out, 1, out) == 0);
        const std::vector<uint8_t> w3 = unhex("00000000000000010000000000000000");
        CHECK(memcmp(out, w3.data(), 16) == 0);
        CHECK(zkaes_ctr_counter_add(nullptr, 1, out) != 0);
    }
    // ---- the ECB fixtures through the CTR verifiers
    const std::vector<uint8_t> vkb = slurp(gold + "/gpu_aes16_vk.bin"), proof = slurp(gold + "/gpu_aes16_proof.bin");
    const std::vector<uint8_t> ecb_ct = unhex("3925841d02dc09fbdc118597196a0b32");          // FIPS-197 appendix B: what the fixture proves under ECB
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
    // the stored key knows its statement has 128 public bits: no CTR length has that many, so every length is an error and nothing is accepted
    for (size_t len : {(size_t)0, (size_t)1, (size_t)15, (size_t)16, (size_t)17, (size_t)64}) {
        acc = 7;
        CHECK(zkaes_verify_encryption_ctr(vk, proof.data(), proof.size(), icb.data(), want.data(), len, &acc) != 0 && acc == 0);
    }
    // the transported key knows |X| = 256 only: lengths that pad to another |X| are rejected by the verifier, 15 bytes (249 inputs) pads to 256 and fails the proof's checks
    for (size_t len : {(size_t)1, (size_t)15, (size_t)16, (size_t)17, (size_t)64}) {
        acc = 7;
        CHECK(zkaes_verify_encryption_ctr(vk_ark, proof.data(), proof.size(), icb.data(), want.data(), len, &acc) == 0 && acc == 0);
    }
    acc = 7;
    CHECK(zkaes_verify_encryption_ctr(vk_ark, proof.data(), proof.size(), icb.data(), want.data(), 0, &acc) != 0 && acc == 0);
    {
        size_t lens[2] = {proof.size(), proof.size()}, n_ok = 9;
        int each[2] = {7, 7};
        std::vector<uint8_t> two(proof);
        two.insert(two.end(), proof.begin(), proof.end());
        CHECK(zkaes_verify_ctr_chunked(vk_ark, two.data(), lens, 2, icb.data(), want.data(), 32, each, &n_ok) == 0 && n_ok == 0 && each[0] == 0 && each[1] == 0);
        CHECK(zkaes_verify_ctr_chunked(vk_ark, two.data(), lens, 1, icb.data(), ecb_ct.data(), 16, nullptr, nullptr) == 0);
        n_ok = 9;
        CHECK(zkaes_verify_ctr_chunked(vk, two.data(), lens, 2, icb.data(), want.data(), 32, each, &n_ok) != 0 && n_ok == 0);        // the key's length is not 16
        CHECK(zkaes_verify_ctr_chunked(vk_ark, two.data(), lens, 2, icb.data(), want.data(), 48, each, &n_ok) != 0 && n_ok == 0);    // 48 bytes are not 2 x whole blocks
        CHECK(zkaes_verify_ctr_chunked(vk_ark, two.data(), lens, 2, icb.data(), want.data(), 34, each, &n_ok) != 0);                 // a chunked job has whole-block chunks
        CHECK(zkaes_verify_ctr_chunked(vk_ark, two.data(), lens, 0, icb.data(), want.data(), 32, each, &n_ok) != 0);
        CHECK(zkaes_verify_ctr_chunked(vk_ark, two.data(), lens, 2, icb.data(), want.data(), 0, each, &n_ok) != 0);
    }
    for (size_t cut = 0; cut < proof.size(); cut++) {                                           // every truncation, in a heap buffer of exactly that size
        std::vector<uint8_t> t(proof.begin(), proof.begin() + cut);
        if (t.empty()) t.reserve(1);
        acc = 7;
        int rc = zkaes_verify_encryption_ctr(vk_ark, t.data() ? t.data() : proof.data(), cut, icb.data(), ecb_ct.data(), 16, &acc);
        CHECK(rc != 0 && acc == 0);
        size_t lens[1] = {cut}, n_ok = 9;
        int each[1] = {7};
        rc = zkaes_verify_ctr_chunked(vk_ark, t.data() ? t.data() : proof.data(), lens, 1, icb.data(), ecb_ct.data(), 16, each, &n_ok);
        CHECK(rc == 0 && n_ok == 0 && each[0] == 0);                                            // an unparsable chunk is a rejected chunk
    }
    zkaes_vk_free(vk);
    zkaes_vk_free(vk_ark);
    if (fails) { fprintf(stderr, "ctr_host_check: %d failure(s)\n", fails); return 1; }
    printf("ctr_host_check ok\n");
    return 0;
}
