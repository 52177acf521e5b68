// tests/verify_batch_keys_host_check.cpp -- stand-alone mutation check of zkaes_verify_batch_keys (the multi-key batch verifier's host back end), built by
// tests/test_verify_batch_keys_host.py with -fsanitize=address,undefined together with csrc/circuit.cpp, csrc/marlin_codec.cpp and csrc/capi_host.cpp (no HIP, no GPU).
// Every batch is the committed GPU-made ECB proof three times under TWO handles of the golden key (two deserializations: two key slots with their own index
// commitments among the bases), rows [true ciphertext, true, wrong ciphertext], with mutations of key_of, of n_bits_each, of the proofs' bytes, of their lengths and of
// the boundaries between slots -- keys, key indices, proofs, lengths, rows, row lengths and answers each in a heap buffer of exactly its size, so that the sanitizer
// watches both ends.  Expected of every call:
//   * no sanitizer report; an error return exactly when a key index is out of range (what the proof BYTES and the rows hold is never an error of the call);
//   * a slot is accepted only if it still holds the golden proof against the true ciphertext at a row length that pads to the key's |X| (anything else is a forgery);
//   * such a slot IS accepted, whatever the other slots hold and whichever handle it names.
// usage: verify_batch_keys_host_check <directory of the golden fixtures> <batches> [seed].  Prints "verify_batch_keys_host_check: N batches ok" and exits 0, or says what
// went wrong.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "../include/zkaes.h"

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
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s <golden dir> <batches> [seed]\n", argv[0]); return 1; }
    const std::string gold = argv[1];
    const long batches = atol(argv[2]);
    if (argc > 3) { rng_state ^= (uint64_t)atol(argv[3]) * 0xbf58476d1ce4e5b9ull; if (!rng_state) rng_state = 1; for (int i = 0; i < 8; i++) rnd(); }
    const std::vector<uint8_t> proof = slurp(gold + "/gpu_aes16_proof.bin"), vkb = slurp(gold + "/gpu_aes16_vk.bin");
    zkaes_vk *vk[2] = {nullptr, nullptr};
    for (int k = 0; k < 2; k++) if (zkaes_vk_deserialize(vkb.data(), vkb.size(), &vk[k])) { fprintf(stderr, "vk: %s\n", zkaes_last_error()); return 1; }
    const uint8_t ct[16] = {0x39, 0x25, 0x84, 0x1d, 0x02, 0xdc, 0x09, 0xfb, 0xdc, 0x11, 0x85, 0x97, 0x19, 0x6a, 0x0b, 0x32};      // FIPS-197 appendix B
    uint8_t true_row[128], wrong_row[128];
    for (int i = 0; i < 128; i++) { true_row[i] = (ct[i / 8] >> (i % 8)) & 1; wrong_row[i] = true_row[i]; }
    wrong_row[77] ^= 1;
    const size_t N = 3, L = proof.size();
    long accepted_total = 0, full_checks = 0, refused = 0;
    for (long it = 0; it < batches; it++) {
        // ---- the batch: three slots, each the golden proof or a mutation of it, each with its own key index and its own row length
        std::vector<std::vector<uint8_t>> slot(N, proof);
        bool golden[N] = {true, true, true};
        size_t n_bits[N] = {128, 128, 128};
        uint32_t key_of[N];
        for (size_t i = 0; i < N; i++) key_of[i] = (uint32_t)(rnd() % 2);
        // The mix (as verify_batch_host_check.cpp's): most batches die in the parser or at a point check; about one in ten keeps a slot alive up to the MSMs, the pairing
        // and the bisection.  Mode 0 mutates the row lengths, mode 2 the key indices
        const unsigned mode = (unsigned)(rnd() % 16);
        if (mode == 0) {                                         // row lengths, per slot: counts that do not fit the key, and two that pad to the same |X|
            static const size_t alt[] = {0, 1, 127, 256, 257, 1000, 129, 200, 128, 128};
            for (size_t i = 0; i < N; i++) n_bits[i] = alt[rnd() % 10];
        }
        bool bad_index = false;
        if (mode == 2) {                                         // a key index past the keys: an error of the call
            static const uint32_t far[] = {2, 3, 0x7fffffffu, 0xffffffffu};
            key_of[rnd() % N] = far[rnd() % 4];
            bad_index = true;
        }
        const size_t head = L - (131 + 8 + 3 + 8 + 4 * 32);      // the commitments: length prefixes, 11 compressed points, Option tags
        for (size_t i = 0; i < N; i++) {
            const unsigned m = mode == 0 || mode == 2 ? 99 : mode == 1 ? (unsigned)(rnd() % 40) : (unsigned)(rnd() % 20);
            if (m <= 7 || m == 19) {                             // one to four bytes, in the commitments (m <= 7) or anywhere (19: the evaluations and openings too)
                const int k = 1 + (int)(rnd() % 4);
                for (int j = 0; j < k; j++) { const size_t at = rnd() % (m == 19 ? L : head); const uint8_t x = (uint8_t)(1 + rnd() % 255); slot[i][at] ^= x; }
                golden[i] = false;
            } else if (m <= 11) { slot[i].resize(rnd() % L); golden[i] = false; }                                         // truncated, down to empty
            else if (m <= 14) { const size_t extra = 1 + rnd() % 64; for (size_t j = 0; j < extra; j++) slot[i].push_back((uint8_t)rnd()); golden[i] = false; }      // trailing bytes
            else if (m <= 16) { for (auto &b : slot[i]) b = (uint8_t)rnd(); golden[i] = false; }                         // garbage of the right length
            else if (m <= 18 && i + 1 < N) {                     // the boundary between two slots moved: both lengths wrong, every byte still there
                const size_t k = 1 + rnd() % 100;
                slot[i + 1].insert(slot[i + 1].begin(), slot[i].end() - k, slot[i].end());
                slot[i].resize(slot[i].size() - k);
                golden[i] = golden[i + 1] = false;
            }                                                    // (m >= 20, mode 1 only: the slot stays golden)
        }
        // ---- exactly sized heap buffers
        size_t total = 0, total_bits = 0;
        for (auto &s : slot) total += s.size();
        for (size_t i = 0; i < N; i++) total_bits += n_bits[i];
        std::unique_ptr<uint8_t[]> proofs(new uint8_t[total ? total : 1]);
        std::unique_ptr<size_t[]> lens(new size_t[N]), row_lens(new size_t[N]);
        std::unique_ptr<uint32_t[]> kof(new uint32_t[N]);
        std::unique_ptr<const zkaes_vk *[]> keys(new const zkaes_vk *[2]);
        keys[0] = vk[0]; keys[1] = vk[1];
        size_t off = 0;
        for (size_t i = 0; i < N; i++) { if (!slot[i].empty()) memcpy(proofs.get() + off, slot[i].data(), slot[i].size()); off += slot[i].size(); lens[i] = slot[i].size(); row_lens[i] = n_bits[i]; kof[i] = key_of[i]; }
        std::unique_ptr<uint8_t[]> bits(new uint8_t[total_bits ? total_bits : 1]);
        off = 0;
        for (size_t i = 0; i < N; i++) {
            for (size_t j = 0; j < n_bits[i]; j++) bits[off + j] = j < 128 ? (i < 2 ? true_row : wrong_row)[j] : (uint8_t)(n_bits[i] == 200 ? 0 : 1);
            off += n_bits[i];
        }
        std::unique_ptr<int[]> each(new int[N]);
        size_t n_ok = 99;
        const int rc = zkaes_verify_batch_keys(keys.get(), 2, kof.get(), proofs.get(), lens.get(), N, total_bits ? bits.get() : nullptr, row_lens.get(), each.get(), &n_ok);
        if (bad_index) {
            if (!rc || !strstr(zkaes_last_error(), "names key")) { fprintf(stderr, "batch %ld: a key index out of range was not refused (%s)\n", it, zkaes_last_error()); return 1; }
            for (size_t i = 0; i < N; i++) if (each[i]) { fprintf(stderr, "batch %ld: a refused call accepted slot %zu\n", it, i); return 1; }
            refused++;
            continue;
        }
        if (rc) { fprintf(stderr, "batch %ld: error return: %s\n", it, zkaes_last_error()); return 1; }
        size_t sum = 0;
        for (size_t i = 0; i < N; i++) {
            // (n_bits = 200 appends zero bits only: the verifier zero-pads to |X| - 1 itself, so that row is the same statement)
            const bool statement = golden[i] && i < 2 && (n_bits[i] == 128 || n_bits[i] == 200);
            if ((each[i] != 0) != statement) { fprintf(stderr, "batch %ld slot %zu: accepted = %d, expected %d (n_bits %zu, key %u)\n", it, i, each[i], (int)statement, n_bits[i], key_of[i]); return 1; }
            sum += each[i] ? 1 : 0;
        }
        if (sum != n_ok) { fprintf(stderr, "batch %ld: n_accepted %zu != %zu\n", it, n_ok, sum); return 1; }
        accepted_total += (long)sum;
        double t[8];
        if (zkaes_verify_batch_timings(t)) return 1;
        full_checks += (long)t[7];
    }
    // null arguments, n = 0 and no key are errors of the call
    size_t one = proof.size(), row = 128;
    uint32_t k0 = 0;
    int e = 0;
    const zkaes_vk *keys[2] = {vk[0], nullptr};
    if (!zkaes_verify_batch_keys(nullptr, 1, &k0, proof.data(), &one, 1, true_row, &row, &e, nullptr) || !zkaes_verify_batch_keys(keys, 0, &k0, proof.data(), &one, 1, true_row, &row, &e, nullptr) ||
        !zkaes_verify_batch_keys(keys, 2, &k0, proof.data(), &one, 1, true_row, &row, &e, nullptr) || !zkaes_verify_batch_keys(keys, 1, nullptr, proof.data(), &one, 1, true_row, &row, &e, nullptr) ||
        !zkaes_verify_batch_keys(keys, 1, &k0, nullptr, &one, 1, true_row, &row, &e, nullptr) || !zkaes_verify_batch_keys(keys, 1, &k0, proof.data(), nullptr, 1, true_row, &row, &e, nullptr) ||
        !zkaes_verify_batch_keys(keys, 1, &k0, proof.data(), &one, 0, true_row, &row, &e, nullptr) || !zkaes_verify_batch_keys(keys, 1, &k0, proof.data(), &one, 1, nullptr, &row, &e, nullptr) ||
        !zkaes_verify_batch_keys(keys, 1, &k0, proof.data(), &one, 1, true_row, nullptr, &e, nullptr)) { fprintf(stderr, "a null argument, n = 0 or no key was not an error\n"); return 1; }
    if (zkaes_verify_batch_keys(keys, 1, &k0, proof.data(), &one, 1, true_row, &row, &e, nullptr) || e != 1) { fprintf(stderr, "the golden statement alone was not accepted\n"); return 1; }
    zkaes_vk_free(vk[0]); zkaes_vk_free(vk[1]);
    printf("verify_batch_keys_host_check: %ld batches ok (%ld slots accepted, %ld pairing checks, %ld calls refused)\n", batches, accepted_total, full_checks, refused);
    return 0;
}
