// tests/gcm_segment_reveal_host_check.cpp -- stand-alone check of the host-only entry points of selective disclosure on segmented GCM records (include/zkaes.h,
// DESIGN.md 9j), built by tests/test_gcm_segments_reveal_host.py with -fsanitize=address,undefined together with csrc/circuit.cpp, csrc/marlin_codec.cpp and
// csrc/capi_host.cpp (no HIP, no GPU):
//   * zkaes_circuit_info_gcm_seg_rv at reveal 0 equals zkaes_circuit_info_gcm_seg, grows by 8 ceil(len / 8) + 8 len instance variables, 16 ceil(len / 8) + 15 len rows and
//     no witness with reveal 1, and refuses reveal 2; zkaes_circuit_matrix_gcm_seg_rv the same;
//   * zkaes_verify_gcm_segments_reveal, fed the committed ECB verifying key and proof as the head and tail of a 17-byte record at c = 1: the key as stored (it knows its
//     128 public bits: an error), after the ark transport (|X| = 256: no segment fits, both rejected), and the ark image with |X| patched to 1024, which a head of 16
//     bytes and a tail of 1 byte with their mask and revealed bits do fit -- there the proof is parsed and checked, whole, truncated at every length and as garbage: a
//     segment that does not parse is a rejected segment, not an error;
//   * under every key: a mask one byte short, a revealed array one byte short, a mask bit at or beyond the record's length and a non-zero revealed byte under a zero mask
//     bit are ERRORS of the call.
// Nothing is ever accepted.  Every buffer is a heap copy of exactly the bytes that exist.
// usage: gcm_segment_reveal_host_check <directory of the golden fixtures>.  Prints "gcm_segment_reveal_host_check ok" and exits 0, or says what went wrong and exits 1.
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
        const size_t shapes[4][3] = {{ZKAES_SEG_HEAD, 1, 13}, {ZKAES_SEG_MID, 2, 0}, {ZKAES_SEG_TAIL, 7, 0}, {ZKAES_SEG_TAIL, 17, 0}};
        for (const auto &sh : shapes) {
            const int role = (int)sh[0];
            const size_t len = role == ZKAES_SEG_TAIL ? sh[1] : 16 * sh[1], mb = (len + 7) / 8;
            CHECK(zkaes_circuit_info_gcm_seg(role, 128, sh[1], sh[2], a) == 0 && zkaes_circuit_info_gcm_seg_rv(role, 128, 0, sh[1], sh[2], b) == 0 && memcmp(a, b, sizeof a) == 0);
            CHECK(zkaes_circuit_info_gcm_seg_rv(role, 128, 1, sh[1], sh[2], b) == 0 && b[0] == a[0] + 16 * mb + 15 * len && b[1] == a[1] + 8 * mb + 8 * len && b[2] == a[2]);
            CHECK(zkaes_circuit_info_gcm_seg_rv(role, 128, 2, sh[1], sh[2], b) != 0);
        }
        uint64_t rows = 0, nnz = 0, rows1 = 0, nnz1 = 0;
        CHECK(zkaes_circuit_matrix_gcm_seg(ZKAES_SEG_TAIL, 128, 7, 0, 0, &rows, &nnz, nullptr, nullptr, nullptr) == 0);
        CHECK(zkaes_circuit_matrix_gcm_seg_rv(ZKAES_SEG_TAIL, 128, 0, 7, 0, 0, &rows1, &nnz1, nullptr, nullptr, nullptr) == 0 && rows1 == rows && nnz1 == nnz);
        CHECK(zkaes_circuit_matrix_gcm_seg_rv(ZKAES_SEG_TAIL, 128, 1, 7, 0, 0, &rows1, &nnz1, nullptr, nullptr, nullptr) == 0 && nnz1 >= nnz + 8 + 56 + 1 + 56);      // A: booleanity of 8 mask and 56 revealed bits, one pin, 56 products: an entry each at the least
        CHECK(zkaes_circuit_matrix_gcm_seg_rv(ZKAES_SEG_TAIL, 128, 2, 7, 0, 0, &rows1, &nnz1, nullptr, nullptr, nullptr) != 0);
    }
    // ---- the ECB fixtures as head and tail of a 17-byte record, c = 1, no aad
    const std::vector<uint8_t> vkb = slurp(gold + "/gpu_aes16_vk.bin"), proof = slurp(gold + "/gpu_aes16_proof.bin");
    const uint8_t ct_bytes[17] = {0x39, 0x25, 0x84, 0x1d, 0x02, 0xdc, 0x09, 0xfb, 0xdc, 0x11, 0x85, 0x97, 0x19, 0x6a, 0x0b, 0x32, 0x39};
    const uint8_t pt_bytes[17] = {0x32, 0x43, 0xf6, 0xa8, 0x88, 0x5a, 0x30, 0x8d, 0x31, 0x31, 0x98, 0xa2, 0xe0, 0x37, 0x07, 0x34, 0x32};
    const uint8_t iv12[12] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12}, tag16[16] = {16, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1};
    const uint8_t ones3[3] = {0xff, 0xff, 0x01}, zero32[32] = {0};
    zkaes_vk *vk = nullptr, *vk_ark = nullptr, *vk_1024 = nullptr;
    CHECK(zkaes_vk_deserialize(vkb.data(), vkb.size(), &vk) == 0 && vk);
    if (!vk) return 1;
    {
        uint8_t *ark = nullptr; size_t ark_len = 0;
        CHECK(zkaes_vk_serialize_ark(vk, &ark, &ark_len) == 0 && ark && ark_len > 32);
        CHECK(zkaes_vk_deserialize_ark(ark, ark_len, &vk_ark) == 0 && vk_ark);
        uint64_t ninst = 0;
        for (int i = 0; i < 8; i++) ninst |= (uint64_t)ark[24 + i] << (8 * i);
        CHECK(ninst == 256);
        ark[25] = 0x04; ark[24] = 0x00;                                                         // |X| = 1024: a head of 16 bytes has 656 inputs with its mask and revealed bits, a tail of 1 byte 664
        CHECK(zkaes_vk_deserialize_ark(ark, ark_len, &vk_1024) == 0 && vk_1024);
        zkaes_bytes_free(ark);
    }
    if (!vk_ark || !vk_1024) return 1;
    int acc = 7, each[2] = {7, 7};
    size_t n_acc = 7, lens[2] = {proof.size(), proof.size()};
    std::vector<uint8_t> two(proof);
    two.insert(two.end(), proof.begin(), proof.end());
    CHECK(zkaes_verify_encryption(vk, proof.data(), proof.size(), ct_bytes, 16, &acc) == 0 && acc == 1);            // (the fixtures are what they claim to be)
    auto ct = exact(ct_bytes, 17), com = exact(zero32, 32), iv = exact(iv12, 12), tag = exact(tag16, 16), both = exact(two.data(), two.size());
    auto mask_all = exact(ones3, 3), mask_none = exact(zero32, 3), rev_all = exact(pt_bytes, 17), rev_none = exact(zero32, 17), mask_short = exact(ones3, 2), rev_short = exact(pt_bytes, 16);
    auto call = [&](const zkaes_vk *k, const uint8_t *proofs, const size_t *pl, const uint8_t *mask, size_t mask_len, const uint8_t *rev, size_t rev_len) {
        each[0] = each[1] = 7; n_acc = 7;
        const int rc = zkaes_verify_gcm_segments_reveal(k, nullptr, k, proofs, pl, 2, 1, iv.get(), nullptr, 0, ct.get(), 17, tag.get(), com.get(), 32, mask, mask_len, rev, rev_len, each, &n_acc);
        if (each[0] != 0 || each[1] != 0 || n_acc != 0) { fprintf(stderr, "FAIL: a segment was accepted, or the verdicts were not cleared (%d %d %zu)\n", each[0], each[1], n_acc); fails++; }
        return rc;
    };
    for (int shown = 0; shown < 2; shown++) {                                                    // everything revealed (the true plaintext of the fixture), nothing revealed
        const uint8_t *m = shown ? mask_all.get() : mask_none.get(), *r = shown ? rev_all.get() : rev_none.get();
        CHECK(call(vk, both.get(), lens, m, 3, r, 17) != 0);                                    // the stored key knows its 128 public bits: an error
        CHECK(call(vk_ark, both.get(), lens, m, 3, r, 17) == 0);                                // |X| = 256: rejected, not an error
        CHECK(call(vk_1024, both.get(), lens, m, 3, r, 17) == 0);                               // the statements fit: parsed, checked, rejected
        // the plain verifier, too, never accepts it
        each[0] = each[1] = 7; n_acc = 7;
        CHECK(zkaes_verify_gcm_segments(vk_1024, nullptr, vk_1024, both.get(), lens, 2, 1, iv.get(), nullptr, 0, ct.get(), 17, tag.get(), com.get(), 32, each, &n_acc) == 0 && each[0] == 0 && each[1] == 0 && n_acc == 0);
    }
    for (zkaes_vk *k : {vk, vk_ark, vk_1024}) {                                                  // arguments that do not go together: errors, whatever the key
        uint8_t hidden[3] = {0xfe, 0xff, 0x01}, beyond[3] = {0xff, 0xff, 0x03};
        CHECK(call(k, both.get(), lens, mask_short.get(), 2, rev_all.get(), 17) != 0);          // a mask one byte short
        CHECK(call(k, both.get(), lens, mask_all.get(), 3, rev_short.get(), 16) != 0);          // a revealed array one byte short
        CHECK(call(k, both.get(), lens, beyond, 3, rev_none.get(), 17) != 0);                   // mask bit 17 of a 17-byte record
        CHECK(call(k, both.get(), lens, hidden, 3, rev_all.get(), 17) != 0);                    // revealed[0] != 0 under mask bit 0 = 0
        CHECK(call(k, both.get(), lens, nullptr, 3, rev_all.get(), 17) != 0);
        CHECK(call(k, both.get(), lens, mask_all.get(), 3, nullptr, 17) != 0);
    }
    for (size_t cut = 0; cut < proof.size(); cut++) {                                           // every truncation, in a heap buffer of exactly that size, as the head: the tail is the
        const bool whole = cut % 96 == 0;                                                       // whole proof (parsed and checked) now and then, else one byte that does not parse
        const size_t second = whole ? proof.size() : 1;
        std::vector<uint8_t> t(proof.begin(), proof.begin() + cut);
        t.insert(t.end(), proof.begin(), proof.begin() + second);
        auto buf = exact(t.data(), t.size());
        size_t l2[2] = {cut, second};
        CHECK(call(vk_1024, buf.get(), l2, mask_all.get(), 3, rev_all.get(), 17) == 0);
    }
    srand(0x5e9);
    for (int round = 0; round < 24; round++) {                                                  // garbage of the proof's length, and the proof with one byte changed
        std::vector<uint8_t> g(two);
        if (round & 1) for (auto &b : g) b = (uint8_t)rand(); else g[(size_t)rand() % g.size()] ^= (uint8_t)(1 + rand() % 255);
        auto buf = exact(g.data(), g.size());
        CHECK(call(vk_1024, buf.get(), lens, mask_all.get(), 3, rev_all.get(), 17) == 0);
    }
    zkaes_vk_free(vk);
    zkaes_vk_free(vk_ark);
    zkaes_vk_free(vk_1024);
    if (fails) { fprintf(stderr, "gcm_segment_reveal_host_check: %d failure(s)\n", fails); return 1; }
    printf("gcm_segment_reveal_host_check ok\n");
    return 0;
}
