// tests/gcm_segment_host_check.cpp -- stand-alone check of the host-only GCM segment entry points of include/zkaes.h, built by tests/test_gcm_segments_host.py with
// -fsanitize=address,undefined together with csrc/circuit.cpp, csrc/marlin_codec.cpp and csrc/capi_host.cpp (no HIP, no GPU):
//   * zkaes_gcm_boundaries into heap buffers of exactly 16 (n - 1) bytes: the count alone, segments of one and of two blocks agree where their boundaries coincide, a
//     short buffer, an empty record, c = 0 and null arguments are errors;
//   * zkaes_gcm_commit equals zkaes_sha256_chain over key || zeros || y || salt for 16-, 24- and 32-byte keys, and refuses a 20-byte key;
//   * zkaes_circuit_info_gcm_seg for a mid of one block (769 instance variables) and its refusals: a role that is none, no units, aad on a mid, a key size that is none;
//   * zkaes_verify_gcm_segments, fed the committed ECB verifying key and proof as all three keys of a three-segment record: the key as stored (it knows its 128 public
//     bits: every call is an error), and the ark image with |X| patched to 1024, which the segments of one block do fit -- there every proof is parsed and checked, whole,
//     truncated at every length and as garbage: a proof that does not parse is a rejected segment, not an error.  A commitments array one commitment short (in a heap
//     buffer of exactly its size), a wrong segment count, a missing mid key and null arguments are errors.  Nothing is ever accepted.
// usage: gcm_segment_host_check <directory of the golden fixtures>.  Prints "gcm_segment_host_check ok" and exits 0, or says what went wrong and exits 1.
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
    uint8_t seq[96];
    for (int i = 0; i < 96; i++) seq[i] = (uint8_t)(7 * i + 3);
    const uint8_t iv[12] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
    // ---- the boundaries
    {
        auto msg = exact(seq, 39), key = exact(seq + 40, 16), aad = exact(seq + 60, 5);
        size_t n = 0;
        CHECK(zkaes_gcm_boundaries(msg.get(), 39, key.get(), 16, iv, aad.get(), 5, 1, nullptr, 0, &n) == 0 && n == 3);
        std::unique_ptr<uint8_t[]> y1(new uint8_t[32]), y2(new uint8_t[16]);
        CHECK(zkaes_gcm_boundaries(msg.get(), 39, key.get(), 16, iv, aad.get(), 5, 1, y1.get(), 32, &n) == 0 && n == 3);
        CHECK(zkaes_gcm_boundaries(msg.get(), 39, key.get(), 16, iv, aad.get(), 5, 2, y2.get(), 16, &n) == 0 && n == 2);
        CHECK(memcmp(y1.get() + 16, y2.get(), 16) == 0 && memcmp(y1.get(), y2.get(), 16) != 0);      // the boundary behind block 1 is one value, however the record is cut
        CHECK(zkaes_gcm_boundaries(msg.get(), 32, key.get(), 16, iv, nullptr, 0, 1, y2.get(), 16, &n) == 0 && n == 2);      // whole blocks: the last segment is full
        CHECK(zkaes_gcm_boundaries(msg.get(), 39, key.get(), 16, iv, aad.get(), 5, 1, y1.get(), 31, &n) != 0);
        CHECK(zkaes_gcm_boundaries(msg.get(), 0, key.get(), 16, iv, aad.get(), 5, 1, y1.get(), 32, &n) != 0);
        CHECK(zkaes_gcm_boundaries(msg.get(), 39, key.get(), 16, iv, aad.get(), 5, 0, y1.get(), 32, &n) != 0);
        CHECK(zkaes_gcm_boundaries(msg.get(), 39, key.get(), 20, iv, aad.get(), 5, 1, y1.get(), 32, &n) != 0);
        CHECK(zkaes_gcm_boundaries(nullptr, 39, key.get(), 16, iv, aad.get(), 5, 1, y1.get(), 32, &n) != 0);
        CHECK(zkaes_gcm_boundaries(msg.get(), 39, key.get(), 16, iv, nullptr, 5, 1, y1.get(), 32, &n) != 0);
    }
    // ---- the commitment
    for (size_t kb : {(size_t)16, (size_t)24, (size_t)32}) {
        auto key = exact(seq, kb), y = exact(seq + 32, 16), salt = exact(seq + 48, 16);
        uint8_t blk[64] = {0}, want[32];
        memcpy(blk, seq, kb); memcpy(blk + 32, seq + 32, 32);
        std::unique_ptr<uint8_t[]> com(new uint8_t[32]);
        CHECK(zkaes_sha256_chain(nullptr, blk, 64, want) == 0 && zkaes_gcm_commit(key.get(), kb, y.get(), salt.get(), com.get()) == 0 && memcmp(com.get(), want, 32) == 0);
        CHECK(zkaes_gcm_commit(key.get(), kb, y.get(), salt.get(), nullptr) != 0 && zkaes_gcm_commit(key.get(), kb, nullptr, salt.get(), com.get()) != 0);
    }
    {
        uint8_t com[32];
        CHECK(zkaes_gcm_commit(seq, 20, seq, seq, com) != 0);
    }
    // ---- circuit queries
    {
        uint64_t a[12], rows = 0, nnz = 0;
        CHECK(zkaes_circuit_info_gcm_seg(ZKAES_SEG_MID, 128, 1, 0, a) == 0 && a[1] == 1 + 128 + 128 + 512 && a[7] == 1024);
        CHECK(zkaes_circuit_info_gcm_seg(3, 128, 1, 0, a) != 0 && zkaes_circuit_info_gcm_seg(-1, 128, 1, 0, a) != 0);
        CHECK(zkaes_circuit_info_gcm_seg(ZKAES_SEG_HEAD, 128, 0, 0, a) != 0 && zkaes_circuit_info_gcm_seg(ZKAES_SEG_TAIL, 128, 0, 0, a) != 0);
        CHECK(zkaes_circuit_info_gcm_seg(ZKAES_SEG_MID, 128, 1, 5, a) != 0 && zkaes_circuit_info_gcm_seg(ZKAES_SEG_TAIL, 128, 7, 5, a) != 0);
        CHECK(zkaes_circuit_info_gcm_seg(ZKAES_SEG_MID, 100, 1, 0, a) != 0);
        CHECK(zkaes_circuit_matrix_gcm_seg(3, 128, 1, 0, 0, &rows, &nnz, nullptr, nullptr, nullptr) != 0);
        CHECK(zkaes_circuit_info(ZKAES_CIRCUIT_AES_GCM_SEG, 16, a) != 0);                          // the generic query has no role to give
    }
    // ---- the ECB fixtures through the segment verifier
    const std::vector<uint8_t> vkb = slurp(gold + "/gpu_aes16_vk.bin"), proof = slurp(gold + "/gpu_aes16_proof.bin");
    zkaes_vk *vk = nullptr, *vk_1024 = nullptr;
    CHECK(zkaes_vk_deserialize(vkb.data(), vkb.size(), &vk) == 0 && vk);
    if (!vk) return 1;
    {
        uint8_t *ark = nullptr; size_t ark_len = 0;
        CHECK(zkaes_vk_serialize_ark(vk, &ark, &ark_len) == 0 && ark && ark_len > 32);
        ark[25] = 0x04; ark[24] = 0x00;                                                         // |X| = 1024: the shape of every segment of one block
        CHECK(zkaes_vk_deserialize_ark(ark, ark_len, &vk_1024) == 0 && vk_1024);
        zkaes_bytes_free(ark);
    }
    if (!vk_1024) return 1;
    auto ct = exact(seq, 39), tag = exact(seq + 40, 16), coms = exact(seq + 16, 64), short_coms = exact(seq + 16, 32);
    int each[3] = {7, 7, 7};
    size_t n_acc = 7, lens[3] = {proof.size(), proof.size(), proof.size()};
    std::vector<uint8_t> three;
    for (int i = 0; i < 3; i++) three.insert(three.end(), proof.begin(), proof.end());
    // the stored key knows its 128 public bits, which no segment has: an error, nothing accepted
    CHECK(zkaes_verify_gcm_segments(vk, vk, vk, three.data(), lens, 3, 1, iv, nullptr, 0, ct.get(), 39, tag.get(), coms.get(), 64, each, &n_acc) != 0 && each[0] == 0 && each[1] == 0 && each[2] == 0 && n_acc == 0);
    // |X| = 1024: all three segments of the 39-byte record fit, so every proof is parsed and checked -- and fails
    each[0] = each[1] = each[2] = 7; n_acc = 7;
    CHECK(zkaes_verify_gcm_segments(vk_1024, vk_1024, vk_1024, three.data(), lens, 3, 1, iv, nullptr, 0, ct.get(), 39, tag.get(), coms.get(), 64, each, &n_acc) == 0 && each[0] == 0 && each[1] == 0 && each[2] == 0 && n_acc == 0);
    CHECK(zkaes_verify_gcm_segments(vk_1024, vk_1024, vk_1024, three.data(), lens, 3, 1, iv, nullptr, 0, ct.get(), 39, tag.get(), coms.get(), 64, nullptr, nullptr) == 0);
    CHECK(zkaes_verify_gcm_segments(vk_1024, nullptr, vk_1024, three.data(), lens, 2, 2, iv, nullptr, 0, ct.get(), 39, tag.get(), short_coms.get(), 32, each, &n_acc) == 0 && each[0] == 0 && each[1] == 0 && n_acc == 0);
    // what does not go together: a commitments array one short, a wrong segment count, no mid key for three segments, c = 0, an empty record, null arguments
    each[0] = each[1] = each[2] = 7; n_acc = 7;
    CHECK(zkaes_verify_gcm_segments(vk_1024, vk_1024, vk_1024, three.data(), lens, 3, 1, iv, nullptr, 0, ct.get(), 39, tag.get(), short_coms.get(), 32, each, &n_acc) != 0 && each[0] == 0 && each[1] == 0 && each[2] == 0 && n_acc == 0);
    CHECK(zkaes_verify_gcm_segments(vk_1024, vk_1024, vk_1024, three.data(), lens, 3, 1, iv, nullptr, 0, ct.get(), 39, tag.get(), coms.get(), 96, each, &n_acc) != 0 && n_acc == 0);
    CHECK(zkaes_verify_gcm_segments(vk_1024, vk_1024, vk_1024, three.data(), lens, 2, 1, iv, nullptr, 0, ct.get(), 39, tag.get(), short_coms.get(), 32, each, &n_acc) != 0 && n_acc == 0);
    CHECK(zkaes_verify_gcm_segments(vk_1024, nullptr, vk_1024, three.data(), lens, 3, 1, iv, nullptr, 0, ct.get(), 39, tag.get(), coms.get(), 64, each, &n_acc) != 0 && n_acc == 0);
    CHECK(zkaes_verify_gcm_segments(vk_1024, vk_1024, vk_1024, three.data(), lens, 3, 0, iv, nullptr, 0, ct.get(), 39, tag.get(), coms.get(), 64, each, &n_acc) != 0);
    CHECK(zkaes_verify_gcm_segments(vk_1024, vk_1024, vk_1024, three.data(), lens, 1, 4, iv, nullptr, 0, ct.get(), 39, tag.get(), coms.get(), 0, each, &n_acc) != 0);       // one segment: the lone key's business
    CHECK(zkaes_verify_gcm_segments(vk_1024, vk_1024, vk_1024, three.data(), lens, 3, 1, iv, nullptr, 0, ct.get(), 0, tag.get(), coms.get(), 64, each, &n_acc) != 0);
    CHECK(zkaes_verify_gcm_segments(vk_1024, vk_1024, vk_1024, three.data(), lens, 3, 1, iv, nullptr, 3, ct.get(), 39, tag.get(), coms.get(), 64, each, &n_acc) != 0);
    CHECK(zkaes_verify_gcm_segments(nullptr, vk_1024, vk_1024, three.data(), lens, 3, 1, iv, nullptr, 0, ct.get(), 39, tag.get(), coms.get(), 64, each, &n_acc) != 0);
    CHECK(zkaes_verify_gcm_segments(vk_1024, vk_1024, vk_1024, three.data(), lens, 3, 1, iv, nullptr, 0, ct.get(), 39, tag.get(), nullptr, 64, each, &n_acc) != 0);
    CHECK(zkaes_verify_gcm_segments(vk_1024, vk_1024, vk_1024, nullptr, lens, 3, 1, iv, nullptr, 0, ct.get(), 39, tag.get(), coms.get(), 64, each, &n_acc) != 0);
    for (size_t cut = 0; cut < proof.size(); cut++) {                                           // every truncation, in a heap buffer of exactly that size, as the mid of three: head and
        const bool whole = cut % 96 == 0;                                                       // tail are the whole proof (parsed and checked) now and then, else one byte that does not parse
        const size_t other = whole ? proof.size() : 1;
        std::vector<uint8_t> t(proof.begin(), proof.begin() + other);
        t.insert(t.end(), proof.begin(), proof.begin() + cut);
        t.insert(t.end(), proof.begin(), proof.begin() + other);
        auto buf = exact(t.data(), t.size());
        size_t l3[3] = {other, cut, other};
        each[0] = each[1] = each[2] = 7; n_acc = 7;
        CHECK(zkaes_verify_gcm_segments(vk_1024, vk_1024, vk_1024, buf.get(), l3, 3, 1, iv, nullptr, 0, ct.get(), 39, tag.get(), coms.get(), 64, each, &n_acc) == 0 && each[0] == 0 && each[1] == 0 && each[2] == 0 && n_acc == 0);
    }
    srand(0x5e9);
    for (int round = 0; round < 16; round++) {                                                  // garbage of the proof's length, and the proof with one byte changed, as the tail of two
        std::vector<uint8_t> g(proof);
        if (round & 1) for (auto &b : g) b = (uint8_t)rand(); else g[(size_t)rand() % g.size()] ^= (uint8_t)(1 + rand() % 255);
        std::vector<uint8_t> t(proof);
        t.insert(t.end(), g.begin(), g.end());
        auto buf = exact(t.data(), t.size());
        each[0] = each[1] = 7; n_acc = 7;
        CHECK(zkaes_verify_gcm_segments(vk_1024, nullptr, vk_1024, buf.get(), lens, 2, 1, iv, nullptr, 0, ct.get(), 32, tag.get(), short_coms.get(), 32, each, &n_acc) == 0 && each[0] == 0 && each[1] == 0 && n_acc == 0);
    }
    zkaes_vk_free(vk);
    zkaes_vk_free(vk_1024);
    if (fails) { fprintf(stderr, "gcm_segment_host_check: %d failure(s)\n", fails); return 1; }
    printf("gcm_segment_host_check ok\n");
    return 0;
}
