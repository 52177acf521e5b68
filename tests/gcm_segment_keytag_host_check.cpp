// tests/gcm_segment_keytag_host_check.cpp -- stand-alone check of the host-only entry points of key tags on segmented GCM records (include/zkaes.h),
// built by tests/test_gcm_segments_keytag_host.py with -fsanitize=address,undefined together with csrc/circuit.cpp, csrc/marlin_codec.cpp and csrc/capi_host.cpp (no
// HIP, no GPU):
//   * zkaes_circuit_info_gcm_seg_kt at T = 0 equals zkaes_circuit_info_gcm_seg_rv for the three roles, grows a head by 128 T instance variables and 9e's rows and
//     witnesses, refuses T = 3 and a mid or tail with T != 0; zkaes_circuit_matrix_gcm_seg_kt the same;
//   * zkaes_gcm_segment_public_inputs_kt into exactly sized buffers: the head's row grows by 8 key_tag_len bits, the tail's does not; a tag of 15 bytes is an error;
//   * zkaes_verify_gcm_segments_kt and zkaes_verify_gcm_segments_batch_kt (plain and with a mask), fed the committed ECB verifying key and proof as the head and tail of
//     a 17-byte record at c = 1: the key as stored (it knows its 128 public bits: an error), after the ark transport (|X| = 256: no segment fits, both rejected), and the
//     ark image with |X| patched to 1024, which a head of 16 bytes with a tag of 16 or 32 bytes and a tail of 1 byte do fit -- there the proof is parsed and checked,
//     whole, truncated at every length and as garbage: a segment that does not parse is a rejected segment, not an error;
//   * under every key: a tag one byte short, no tag, and a commitments array one short are ERRORS of the call.
// Nothing is ever accepted.  Every buffer is a heap copy of exactly the bytes that exist.
// usage: gcm_segment_keytag_host_check <directory of the golden fixtures>.  Prints "gcm_segment_keytag_host_check ok" and exits 0, or says what went wrong and exits 1.
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
        const size_t shapes[3][3] = {{ZKAES_SEG_HEAD, 1, 13}, {ZKAES_SEG_MID, 1, 0}, {ZKAES_SEG_TAIL, 7, 0}};
        for (const auto &sh : shapes) {
            const int role = (int)sh[0];
            for (unsigned rv = 0; rv < 2; rv++) {
                CHECK(zkaes_circuit_info_gcm_seg_rv(role, 128, rv, sh[1], sh[2], a) == 0 && zkaes_circuit_info_gcm_seg_kt(role, 128, rv, 0, sh[1], sh[2], b) == 0 && memcmp(a, b, sizeof a) == 0);
                for (unsigned T = 1; T <= 2; T++) {
                    const int rc = zkaes_circuit_info_gcm_seg_kt(role, 128, rv, T, sh[1], sh[2], b);
                    if (role == ZKAES_SEG_HEAD) CHECK(rc == 0 && b[0] == a[0] + 148016 * T && b[1] == a[1] + 128 * T && b[2] == a[2] + 147760 * T);
                    else CHECK(rc != 0 && strstr(zkaes_last_error(), "the head carries") && strstr(zkaes_last_error(), "commitments carry the key"));
                }
                CHECK(zkaes_circuit_info_gcm_seg_kt(role, 128, rv, 3, sh[1], sh[2], b) != 0);
            }
        }
        uint64_t rows = 0, nnz = 0, rows1 = 0, nnz1 = 0;
        CHECK(zkaes_circuit_matrix_gcm_seg(ZKAES_SEG_HEAD, 128, 1, 5, 0, &rows, &nnz, nullptr, nullptr, nullptr) == 0);
        CHECK(zkaes_circuit_matrix_gcm_seg_kt(ZKAES_SEG_HEAD, 128, 0, 0, 1, 5, 0, &rows1, &nnz1, nullptr, nullptr, nullptr) == 0 && rows1 == rows && nnz1 == nnz);
        CHECK(zkaes_circuit_matrix_gcm_seg_kt(ZKAES_SEG_HEAD, 128, 0, 1, 1, 5, 0, &rows1, &nnz1, nullptr, nullptr, nullptr) == 0 && nnz1 > nnz + 128);
        CHECK(zkaes_circuit_matrix_gcm_seg_kt(ZKAES_SEG_HEAD, 128, 0, 3, 1, 5, 0, &rows1, &nnz1, nullptr, nullptr, nullptr) != 0);
        CHECK(zkaes_circuit_matrix_gcm_seg_kt(ZKAES_SEG_TAIL, 128, 0, 1, 7, 0, 0, &rows1, &nnz1, nullptr, nullptr, nullptr) != 0);
    }
    // ---- the ECB fixtures as head and tail of a 17-byte record, c = 1, no aad
    const std::vector<uint8_t> vkb = slurp(gold + "/gpu_aes16_vk.bin"), proof = slurp(gold + "/gpu_aes16_proof.bin");
    const uint8_t ct_bytes[17] = {0x39, 0x25, 0x84, 0x1d, 0x02, 0xdc, 0x09, 0xfb, 0xdc, 0x11, 0x85, 0x97, 0x19, 0x6a, 0x0b, 0x32, 0x39};
    const uint8_t pt_bytes[17] = {0x32, 0x43, 0xf6, 0xa8, 0x88, 0x5a, 0x30, 0x8d, 0x31, 0x31, 0x98, 0xa2, 0xe0, 0x37, 0x07, 0x34, 0x32};
    const uint8_t iv12[12] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12}, tag16[16] = {16, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1};
    const uint8_t ones3[3] = {0xff, 0xff, 0x01}, zero32[32] = {0};
    uint8_t kt_bytes[32];
    CHECK(zkaes_key_tag(pt_bytes, 16, 2, kt_bytes) == 0);                                        // any 32 bytes would do: these are a real tag
    auto ct = exact(ct_bytes, 17), com = exact(zero32, 32), iv = exact(iv12, 12), tag = exact(tag16, 16), kt16 = exact(kt_bytes, 16), kt32 = exact(kt_bytes, 32), kt15 = exact(kt_bytes, 15);
    auto mask_all = exact(ones3, 3), rev_all = exact(pt_bytes, 17);
    // ---- the rows, into exactly sized buffers
    {
        size_t n_plain[2] = {0, 0}, n_kt[2] = {0, 0};
        int roles[2] = {7, 7};
        CHECK(zkaes_gcm_segment_public_inputs(2, 1, iv.get(), nullptr, 0, ct.get(), 17, tag.get(), com.get(), 32, nullptr, 0, nullptr, nullptr, n_plain, roles) == 0 && roles[0] == 0 && roles[1] == 2);
        for (size_t kl : {(size_t)16, (size_t)32}) {
            CHECK(zkaes_gcm_segment_public_inputs_kt(2, 1, iv.get(), nullptr, 0, ct.get(), 17, tag.get(), com.get(), 32, kl == 16 ? kt16.get() : kt32.get(), kl, nullptr, 0, nullptr, nullptr, n_kt, roles) == 0);
            CHECK(n_kt[0] == n_plain[0] + 8 * kl && n_kt[1] == n_plain[1] && n_plain[0] == 512 && n_plain[1] == 648);
            std::unique_ptr<uint8_t[]> rows(new uint8_t[n_kt[0] + n_kt[1]]), plain(new uint8_t[n_plain[0] + n_plain[1]]);
            CHECK(zkaes_gcm_segment_public_inputs_kt(2, 1, iv.get(), nullptr, 0, ct.get(), 17, tag.get(), com.get(), 32, kl == 16 ? kt16.get() : kt32.get(), kl, nullptr, 0, nullptr, rows.get(), n_kt, roles) == 0);
            CHECK(zkaes_gcm_segment_public_inputs(2, 1, iv.get(), nullptr, 0, ct.get(), 17, tag.get(), com.get(), 32, nullptr, 0, nullptr, plain.get(), n_plain, roles) == 0);
            CHECK(memcmp(rows.get(), plain.get(), 512) == 0 && memcmp(rows.get() + n_kt[0], plain.get() + 512, 648) == 0);      // head ahead of the tag and the whole tail: unchanged
            for (size_t i = 0; i < 8 * kl; i++) if (rows[512 + i] != ((kt_bytes[i / 8] >> (i % 8)) & 1)) { fprintf(stderr, "FAIL: tag bit %zu of the head row\n", i); fails++; break; }
            // with a mask the tag stays ahead of it
            CHECK(zkaes_gcm_segment_public_inputs_kt(2, 1, iv.get(), nullptr, 0, ct.get(), 17, tag.get(), com.get(), 32, kt16.get(), 16, mask_all.get(), 3, rev_all.get(), nullptr, n_kt, roles) == 0 &&
                  n_kt[0] == 512 + 128 + 16 + 128 && n_kt[1] == 648 + 8 + 8);
        }
        CHECK(zkaes_gcm_segment_public_inputs_kt(2, 1, iv.get(), nullptr, 0, ct.get(), 17, tag.get(), com.get(), 32, kt15.get(), 15, nullptr, 0, nullptr, nullptr, n_kt, roles) != 0);
        CHECK(zkaes_gcm_segment_public_inputs_kt(2, 1, iv.get(), nullptr, 0, ct.get(), 17, tag.get(), com.get(), 32, nullptr, 16, nullptr, 0, nullptr, nullptr, n_kt, roles) != 0);
        CHECK(zkaes_gcm_segment_public_inputs_kt(2, 1, iv.get(), nullptr, 0, ct.get(), 17, tag.get(), com.get(), 31, kt16.get(), 16, nullptr, 0, nullptr, nullptr, n_kt, roles) != 0);
    }
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
        ark[25] = 0x04; ark[24] = 0x00;                                                         // |X| = 1024: a head of 16 bytes has 640 or 768 inputs with its tag, a tail of 1 byte 648
        CHECK(zkaes_vk_deserialize_ark(ark, ark_len, &vk_1024) == 0 && vk_1024);
        zkaes_bytes_free(ark);
    }
    if (!vk_ark || !vk_1024) return 1;
    int acc = 7, each[2] = {7, 7};
    size_t n_acc = 7, lens[2] = {proof.size(), proof.size()};
    std::vector<uint8_t> two(proof);
    two.insert(two.end(), proof.begin(), proof.end());
    CHECK(zkaes_verify_encryption(vk, proof.data(), proof.size(), ct_bytes, 16, &acc) == 0 && acc == 1);            // (the fixtures are what they claim to be)
    auto both = exact(two.data(), two.size());
    // form 0: the per-proof verifier, 1: the batch verifier; with_mask: the reveal statement behind the tag
    auto call = [&](int form, const zkaes_vk *k, const uint8_t *proofs, const size_t *pl, const uint8_t *kt, size_t kt_len, size_t com_len, bool with_mask) {
        each[0] = each[1] = 7; n_acc = 7;
        const uint8_t *m = with_mask ? mask_all.get() : nullptr, *r = with_mask ? rev_all.get() : nullptr;
        const int rc = (form ? zkaes_verify_gcm_segments_batch_kt : zkaes_verify_gcm_segments_kt)(k, nullptr, k, proofs, pl, 2, 1, iv.get(), nullptr, 0, ct.get(), 17, tag.get(), com.get(), com_len, kt, kt_len,
                                                                                                   m, with_mask ? 3 : 0, r, with_mask ? 17 : 0, each, &n_acc);
        if (each[0] != 0 || each[1] != 0 || n_acc != 0) { fprintf(stderr, "FAIL: a segment was accepted, or the verdicts were not cleared (%d %d %zu)\n", each[0], each[1], n_acc); fails++; }
        return rc;
    };
    for (int form = 0; form < 2; form++) for (int with_mask = 0; with_mask < 2; with_mask++) {
        for (size_t kl : {(size_t)16, (size_t)32}) {
            const uint8_t *kt = kl == 16 ? kt16.get() : kt32.get();
            CHECK(call(form, vk, both.get(), lens, kt, kl, 32, with_mask) != 0);                  // the stored key knows its 128 public bits: an error
            CHECK(call(form, vk_ark, both.get(), lens, kt, kl, 32, with_mask) == 0);              // |X| = 256: the head does not fit its tag: rejected, not an error
            CHECK(call(form, vk_1024, both.get(), lens, kt, kl, 32, with_mask) == 0);             // the statements fit: parsed, checked, rejected
        }
        for (zkaes_vk *k : {vk, vk_ark, vk_1024}) {                                                // arguments that do not go together: errors, whatever the key
            CHECK(call(form, k, both.get(), lens, kt15.get(), 15, 32, with_mask) != 0);           // a tag one byte short
            CHECK(call(form, k, both.get(), lens, nullptr, 16, 32, with_mask) != 0);              // no tag
            CHECK(call(form, k, both.get(), lens, kt16.get(), 0, 32, with_mask) != 0);
            CHECK(call(form, k, both.get(), lens, kt16.get(), 16, 31, with_mask) != 0);           // a commitments array one short
        }
    }
    for (size_t cut = 0; cut < proof.size(); cut++) {                                           // every truncation, in a heap buffer of exactly that size, as the head: the tail is the
        const bool whole = cut % 96 == 0;                                                       // whole proof (parsed and checked) now and then, else one byte that does not parse
        const size_t second = whole ? proof.size() : 1;
        std::vector<uint8_t> t(proof.begin(), proof.begin() + cut);
        t.insert(t.end(), proof.begin(), proof.begin() + second);
        auto buf = exact(t.data(), t.size());
        size_t l2[2] = {cut, second};
        CHECK(call(0, vk_1024, buf.get(), l2, kt16.get(), 16, 32, false) == 0);
        if (cut % 7 == 0) CHECK(call(1, vk_1024, buf.get(), l2, kt32.get(), 32, 32, false) == 0);
    }
    srand(0x5ea);
    for (int round = 0; round < 24; round++) {                                                  // garbage of the proof's length, and the proof with one byte changed
        std::vector<uint8_t> g(two);
        if (round & 1) for (auto &b : g) b = (uint8_t)rand(); else g[(size_t)rand() % g.size()] ^= (uint8_t)(1 + rand() % 255);
        auto buf = exact(g.data(), g.size());
        CHECK(call(round % 4 / 2, vk_1024, buf.get(), lens, kt16.get(), 16, 32, round % 3 == 0) == 0);
    }
    zkaes_vk_free(vk);
    zkaes_vk_free(vk_ark);
    zkaes_vk_free(vk_1024);
    if (fails) { fprintf(stderr, "gcm_segment_keytag_host_check: %d failure(s)\n", fails); return 1; }
    printf("gcm_segment_keytag_host_check ok\n");
    return 0;
}
