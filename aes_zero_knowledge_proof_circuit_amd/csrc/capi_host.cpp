// csrc/capi_host.cpp -- the host-only entry points of include/zkaes.h: the verifier (src/lib.rs:116-136), proof / verifying-key (de)serialisation, circuit queries.
// No device, no HIP header: this file, marlin_codec.cpp and circuit.cpp are also built with -fsanitize=address,undefined,fuzzer (tests/fuzz_host.cpp).
#include "capi_common.hpp"
#include <algorithm>
#include "statement.hpp"

namespace {
thread_local std::string g_err;
zk::Circuit compile(int kind, size_t len, size_t aad_len = 0, size_t key_bits = 128, size_t key_tag_blocks = 0, int digest_kind = 0, uint64_t digest_prefix = 0, int reveal = 0) {
    return zk::compile_circuit(kind, len, aad_len, key_bits, key_tag_blocks, digest_kind, digest_prefix, reveal);
}
void require_key_len(size_t key_len) { if (key_len != 16 && key_len != 24 && key_len != 32) throw std::invalid_argument("the AES key must have 16, 24 or 32 bytes"); }
// Chunk j's public input without the leading One, as every chunked verifier and zkaes_chunk_public_inputs derive it: the header entering the chunk (statement.hpp, the
// prover's own rule), the chunk's ciphertext bits, the key tag's when there is one, (states[j], states[j + 1]) when there are states, and the chunk's slice of the job's
// mask and of its revealed bytes when there is a mask
std::vector<zk::Fr> chunk_public_input(int circuit_kind, size_t j, size_t chunk, const uint8_t *iv_or_icb, const uint8_t *ct, const uint8_t *key_tag, size_t key_tag_len, const uint8_t *states,
                                       const uint8_t *mask = nullptr, const uint8_t *revealed = nullptr) {
    uint8_t hdr[16];
    const size_t hb = zk::chunk_mode_header(circuit_kind, j, chunk, iv_or_icb, ct, hdr);
    return zk::public_input_of({{hdr, hb}, {ct + chunk * j, chunk}, {key_tag, key_tag_len}, {states ? states + 32 * j : nullptr, 64},      // states[j] is H_in, states[j + 1] H_out
                                {mask ? zk::chunk_mask_slice(mask, j, chunk) : nullptr, zk::mask_bytes(chunk)}, {mask ? revealed + chunk * j : nullptr, chunk}});
}
// a GCM record's public input without the leading One: iv, aad, ciphertext, tag, then the key tag and (h_in, h_out) of the keys that carry them (null otherwise)
std::vector<zk::Fr> gcm_public_input(const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const uint8_t *ct, size_t ct_len, const uint8_t tag[16], const uint8_t *key_tag, size_t key_tag_len,
                                     const uint8_t *h_in, const uint8_t *h_out, const uint8_t *mask = nullptr, const uint8_t *revealed = nullptr) {
    return zk::public_input_of({{iv, 12}, {aad, aad_len}, {ct, ct_len}, {tag, 16}, {key_tag, key_tag_len}, {h_in, 32}, {h_out, 32}, {mask, zk::mask_bytes(ct_len)}, {mask ? revealed : nullptr, ct_len}});
}
// n proofs packed one behind the other, each checked by accept(j, proof): a proof whose bytes do not parse is a rejected proof, not an error of the call
template <class Accept> void verify_each(const uint8_t *proofs, const size_t *proof_lens, size_t n, int *accepted_each, size_t *n_accepted, Accept &&accept) {
    size_t off = 0, ok = 0;
    for (size_t j = 0; j < n; j++) {
        int acc = 0;
        try {
            zk::Proof p = zk::deserialize_proof(proofs + off, proof_lens[j]);
            acc = accept(j, p) ? 1 : 0;
        } catch (const std::runtime_error &) { acc = 0; }
        if (accepted_each) accepted_each[j] = acc;
        ok += (size_t)acc;
        off += proof_lens[j];
    }
    if (n_accepted) *n_accepted = ok;
}
// the chunk-proofs of one ECB, CBC or CTR job of n_chunks slices of `chunk` bytes, chunk j against chunk_public_input(j)
void verify_chunks(const zk::VerifyingKey &vk, int circuit_kind, const uint8_t *proofs, const size_t *proof_lens, size_t n_chunks, size_t chunk, const uint8_t *iv_or_icb, const uint8_t *ct,
                   const uint8_t *key_tag, size_t key_tag_len, const uint8_t *states, int *accepted_each, size_t *n_accepted, const uint8_t *mask = nullptr, const uint8_t *revealed = nullptr) {
    verify_each(proofs, proof_lens, n_chunks, accepted_each, n_accepted, [&](size_t j, const zk::Proof &p) {
        return zk::verify(vk, chunk_public_input(circuit_kind, j, chunk, iv_or_icb, ct, key_tag, key_tag_len, states, mask, revealed), p);
    });
}
// ---- GCM segments: segment s's public input, and the one body of zkaes_verify_gcm_segments and zkaes_verify_gcm_segments_reveal (described at the entries)
std::vector<zk::Fr> gcm_segment_public_input(size_t s, size_t n, size_t c, size_t lt, const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const uint8_t *ct, const uint8_t lenblk[16],
                                             const uint8_t tag[16], const uint8_t *commitments, const uint8_t *mask, const uint8_t *revealed, const uint8_t *key_tag = nullptr,
                                             size_t key_tag_len = 0) {
    uint8_t hd[16];
    memcpy(hd, iv, 12);
    const uint32_t ctr0 = (uint32_t)(2 + s * c);
    for (int i = 0; i < 4; i++) hd[12 + i] = (uint8_t)(ctr0 >> (24 - 8 * i));
    const bool first = s == 0, last = s + 1 == n;
    const size_t len = last ? lt : 16 * c;
    return zk::public_input_of({{hd, 16}, {first ? aad : nullptr, aad_len}, {ct + 16 * c * s, len}, {last ? lenblk : nullptr, 16}, {last ? tag : nullptr, 16},
                                {first ? nullptr : commitments + 32 * (s - 1), 32}, {last ? nullptr : commitments + 32 * s, 32}, {first ? key_tag : nullptr, key_tag_len},      // (9l: the head alone carries the tag)
                                {mask ? zk::chunk_mask_slice(mask, s, 16 * c) : nullptr, zk::mask_bytes(len)}, {mask ? revealed + 16 * c * s : nullptr, len}});
}
// what both verifiers of a segmented record and zkaes_gcm_segment_public_inputs check before any proof is looked at: the lengths and counts, and (keys given) that
// the three keys fit them.  Returns n, the tail's bytes and the length block
struct SegShape { size_t n, lt; uint8_t lenblk[16]; bool head_fits; };
SegShape gcm_segments_shape(const char *entry, bool with_keys, const zkaes_vk *head, const zkaes_vk *mid_or_null, const zkaes_vk *tail, size_t n_segments, size_t c, const uint8_t iv[12],
                            const uint8_t *aad, size_t aad_len, const uint8_t *ct, size_t ct_len, const uint8_t tag[16], const uint8_t *commitments, size_t commitments_len, bool reveal,
                            const uint8_t *mask, size_t mask_len, const uint8_t *revealed, size_t revealed_len, const uint8_t *key_tag = nullptr, size_t key_tag_len = 0) {
    if (key_tag ? (key_tag_len != 16 && key_tag_len != 32) : key_tag_len != 0) throw std::invalid_argument(std::string(entry) + ": key_tag_len must be 16 or 32 with a key tag (one or two tag blocks), 0 with NULL");
    if ((with_keys && (!head || !tail)) || !iv || !ct || !tag || !commitments || (aad_len && !aad) || (reveal && (!mask || !revealed))) throw std::invalid_argument("null argument");
    if (c == 0 || ct_len == 0 || ct_len > ((size_t)1 << 20) || aad_len > ((size_t)1 << 16)) throw std::invalid_argument("GCM segments: a record has 1 .. 2^20 bytes, at most 65536 bytes of aad, and a segment at least one block");
    const size_t nb = (ct_len + 15) / 16, n = (nb + c - 1) / c;
    if (n < 2) throw std::invalid_argument("GCM segments: this record fits one segment; a record that fits one proof is checked with zkaes_verify_encryption_gcm");
    if (n_segments != n) throw std::invalid_argument("GCM segments: the record has " + std::to_string(n) + " segments of " + std::to_string(c) + " blocks");
    if (commitments_len != 32 * (n - 1)) throw std::invalid_argument("GCM segments: one 32-byte commitment per boundary, " + std::to_string(32 * (n - 1)) + " bytes for this record");
    if (with_keys && n > 2 && !mid_or_null) throw std::invalid_argument("GCM segments: a record of more than two segments needs the mid key");
    if (reveal) {
        if (mask_len != zk::mask_bytes(ct_len)) throw std::invalid_argument(std::string(entry) + ": ONE mask over the whole record, " + std::to_string(zk::mask_bytes(ct_len)) + " bytes for this ciphertext");
        if (revealed_len != ct_len) throw std::invalid_argument(std::string(entry) + ": ONE revealed array over the whole record, " + std::to_string(ct_len) + " bytes for this ciphertext");
        zk::require_revealed(mask, revealed, ct_len);
    }
    const size_t lt = ct_len - 16 * c * (n - 1);
    // the verifier zero-pads the public input, so the lengths are part of the statement (as require_gcm_lengths): a key that knows its exact count pins them -- and
    // tells a reveal key from a plain one, whose count lacks the mask's and the revealed bytes' bits
    // A head also tells its tag blocks: a tagged head checked without a tag, an untagged one with a tag, or a tag of the other length raises here
    auto exact = [&](const zk::VerifyingKey &vk, size_t bits, size_t len, const char *name, size_t tag_bits = 0, bool is_head = false) {
        if (vk.num_public_inputs + 1 == vk.num_instance) return;
        const size_t rv_bits = 8 * zk::mask_bytes(len) + 8 * len;
        if (is_head && vk.num_public_inputs != bits + tag_bits + (reveal ? rv_bits : 0))
            for (size_t other : {(size_t)0, (size_t)128, (size_t)256})
                if (other != tag_bits && vk.num_public_inputs == bits + other + (reveal ? rv_bits : 0))
                    throw std::invalid_argument(std::string(entry) + ": the head key was synthesized with key_tag_blocks = " + std::to_string(other / 128) + ": it is checked " +
                                                (other ? "against a key tag of " + std::to_string(other / 8) + " bytes (the _kt entries)" : std::string("without a key tag")));
        bits += tag_bits;
        if (vk.num_public_inputs == bits + (reveal ? 0 : rv_bits))
            throw std::invalid_argument(std::string("GCM segments: the ") + name + (reveal ? " key has no reveal region: zkaes_verify_gcm_segments_reveal takes keys synthesized with reveal = 1 (zkaes_verify_gcm_segments checks this one)"
                                                                                           : " key reveals plaintext bytes: its proofs are checked with zkaes_verify_gcm_segments_reveal"));
        // (a verifying key carries its public-input count and no digest flag: a count 512 or 576 bits over is what a segment key of a digest record has, and also what a
        // plain key for other lengths can have, so the message names both)
        const bool dg_count = !reveal && (vk.num_public_inputs == bits + 512 || vk.num_public_inputs == bits + 576);
        if (vk.num_public_inputs != bits + (reveal ? rv_bits : 0))
            throw std::invalid_argument(std::string("GCM segments: the ") + name + " key was not synthesized for this segment's lengths" +
                                        (dg_count ? " (its count fits a segment key of a digest record: those proofs are checked with zkaes_verify_gcm_segments_digest)" : ""));
    };
    if (with_keys) {
        exact(head->vk, 128 + 8 * aad_len + 128 * c + 256, 16 * c, "head", 8 * key_tag_len, true);
        if (n > 2) exact(mid_or_null->vk, 128 + 128 * c + 512, 16 * c, "mid");
        exact(tail->vk, 128 + 8 * lt + 128 + 128 + 256, lt, "tail");
    }
    SegShape S;
    S.n = n; S.lt = lt;
    // a head from the ark transport carries only |X|: a tag whose bits do not pad to it rejects the head segment (9e's rule, fits_key)
    S.head_fits = !with_keys || !key_tag_len || head->vk.num_public_inputs + 1 != head->vk.num_instance ||
                  zk::capi::next_pow2(128 + 8 * aad_len + 128 * c + 256 + 8 * key_tag_len + (reveal ? 8 * zk::mask_bytes(16 * c) + 128 * c : 0) + 1) == head->vk.num_instance;
    uint8_t *lenblk = S.lenblk;
    for (int i = 0; i < 8; i++) { lenblk[i] = (uint8_t)((uint64_t)(8 * aad_len) >> (56 - 8 * i)); lenblk[8 + i] = (uint8_t)((uint64_t)(8 * ct_len) >> (56 - 8 * i)); }
    return S;
}
void verify_gcm_segments(const char *entry, const zkaes_vk *head, const zkaes_vk *mid_or_null, const zkaes_vk *tail, const uint8_t *proofs, const size_t *proof_lens, size_t n_segments, size_t c,
                         const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const uint8_t *ct, size_t ct_len, const uint8_t tag[16], const uint8_t *commitments, size_t commitments_len,
                         bool reveal, const uint8_t *mask, size_t mask_len, const uint8_t *revealed, size_t revealed_len, int *accepted_each, size_t *n_accepted,
                         const uint8_t *key_tag = nullptr, size_t key_tag_len = 0) {
    if (n_accepted) *n_accepted = 0;
    if (accepted_each) for (size_t s = 0; s < n_segments; s++) accepted_each[s] = 0;
    if (!proofs || !proof_lens) throw std::invalid_argument("null argument");
    const SegShape S = gcm_segments_shape(entry, true, head, mid_or_null, tail, n_segments, c, iv, aad, aad_len, ct, ct_len, tag, commitments, commitments_len, reveal, mask, mask_len, revealed,
                                          revealed_len, key_tag, key_tag_len);
    const size_t n = S.n, lt = S.lt;
    const uint8_t *lenblk = S.lenblk;
    verify_each(proofs, proof_lens, n, accepted_each, n_accepted, [&](size_t s, const zk::Proof &p) {
        if (s == 0 && !S.head_fits) return false;
        return zk::verify(s == 0 ? head->vk : s + 1 == n ? tail->vk : mid_or_null->vk,
                          gcm_segment_public_input(s, n, c, lt, iv, aad, aad_len, ct, lenblk, tag, commitments, reveal ? mask : nullptr, revealed, key_tag, key_tag_len), p);
    });
}
// the n rows of one record as 0/1 bytes, one behind the other (ragged: head, mid and tail rows differ in length), through gcm_segment_public_input: what the per-proof
// verifier above checks segment s against.  role: 0 head, 1 mid, 2 tail
void gcm_segment_rows(const SegShape &S, size_t c, const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const uint8_t *ct, const uint8_t tag[16], const uint8_t *commitments,
                      const uint8_t *mask, const uint8_t *revealed, std::vector<uint8_t> *bits, std::vector<size_t> &lens, std::vector<int> &roles, const uint8_t *key_tag = nullptr,
                      size_t key_tag_len = 0) {
    lens.assign(S.n, 0); roles.assign(S.n, 1);
    roles[0] = 0; roles[S.n - 1] = 2;
    for (size_t s = 0; s < S.n; s++) {
        const bool first = s == 0, last = s + 1 == S.n;
        const size_t len = last ? S.lt : 16 * c;
        lens[s] = 128 + (first ? 8 * aad_len : 0) + 8 * len + (last ? 256 : 0) + (first || last ? 256 : 512) + (first ? 8 * key_tag_len : 0) + (mask ? 8 * zk::mask_bytes(len) + 8 * len : 0);
        if (!bits) continue;
        const std::vector<zk::Fr> pub = gcm_segment_public_input(s, S.n, c, S.lt, iv, aad, aad_len, ct, S.lenblk, tag, commitments, mask, revealed, key_tag, key_tag_len);
        if (pub.size() != lens[s]) throw std::logic_error("GCM segments: a segment's public input has not the documented length");
        for (const zk::Fr &v : pub) bits->push_back(v.is_zero() ? 0 : 1);
    }
}
// ---- digests on segmented records: nd data segments (head, mids, last) and the closing tail, nd + 1 proofs.  What the verifier and
// zkaes_gcm_segment_digest_public_inputs check before any proof is looked at, and proof s's public input
struct DgShape { size_t nd, lr; uint8_t lenblk[16], bits[8]; };
DgShape gcm_digest_shape(const char *entry, bool with_keys, const zkaes_vk *head, const zkaes_vk *mid_or_null, const zkaes_vk *last, const zkaes_vk *tail, size_t n_proofs, size_t c,
                         const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const uint8_t *ct, size_t ct_len, const uint8_t tag[16], const uint8_t *commitments, size_t commitments_len,
                         const uint8_t *states, size_t states_len, uint64_t digest_prefix) {
    if ((with_keys && (!head || !last || !tail)) || !iv || !ct || !tag || !commitments || !states || (aad_len && !aad)) throw std::invalid_argument("null argument");
    if (ct_len == 0 || ct_len > ((size_t)1 << 20) || aad_len > ((size_t)1 << 16)) throw std::invalid_argument("GCM segments: a record has 1 .. 2^20 bytes and at most 65536 bytes of aad");
    if (c == 0 || c % 4) throw std::invalid_argument(std::string(entry) + ": a digest segment holds whole 64-byte blocks: c must be a multiple of 4");
    if (ct_len <= 16 * c) throw std::invalid_argument(std::string(entry) + ": this record fits one segment; a record that fits one proof is checked with zkaes_verify_encryption_gcm_digest");
    if (digest_prefix % 64 || digest_prefix >= ((uint64_t)1 << 61) - ct_len) throw std::invalid_argument(std::string(entry) + ": digest_prefix must be a multiple of 64 with digest_prefix + the record's length below 2^61");
    DgShape S;
    S.nd = (ct_len + 16 * c - 1) / (16 * c); S.lr = ct_len - 16 * c * (S.nd - 1);
    if (n_proofs != S.nd + 1) throw std::invalid_argument(std::string(entry) + ": the record has " + std::to_string(S.nd) + " data segments of " + std::to_string(c) + " blocks and the closing tail: " + std::to_string(S.nd + 1) + " proofs");
    if (commitments_len != 32 * S.nd) throw std::invalid_argument(std::string(entry) + ": one 32-byte commitment behind every data segment, " + std::to_string(32 * S.nd) + " bytes for this record");
    if (states_len != 32 * (S.nd + 1)) throw std::invalid_argument(std::string(entry) + ": one 32-byte state per data segment and one more, " + std::to_string(32 * (S.nd + 1)) + " bytes for this record");
    if (with_keys && S.nd > 2 && !mid_or_null) throw std::invalid_argument(std::string(entry) + ": a record of more than two data segments needs the mid key");
    // a key that knows its exact public-input count pins the lengths, and tells a digest segment key from a plain one, whose count lacks the states' bits
    auto exact = [&](const zk::VerifyingKey &vk, size_t plain_bits, size_t dg_bits, const char *name) {
        if (vk.num_public_inputs + 1 == vk.num_instance) return;
        if (dg_bits && vk.num_public_inputs == plain_bits)
            throw std::invalid_argument(std::string(entry) + ": the " + name + " key is a plain segment key: its proofs are checked with zkaes_verify_gcm_segments (digest segment keys come from zkaes_synthesize_keys_gcm_seg_dg)");
        if (vk.num_public_inputs != plain_bits + dg_bits) throw std::invalid_argument(std::string(entry) + ": the " + name + " key was not synthesized for this segment's lengths");
    };
    if (with_keys) {
        exact(head->vk, 128 + 8 * aad_len + 128 * c + 256, 512, "head");
        if (S.nd > 2) exact(mid_or_null->vk, 128 + 128 * c + 512, 512, "mid");
        exact(last->vk, 128 + 8 * S.lr + 512, 512 + 64, "last");
        exact(tail->vk, 128 + 128 + 128 + 256, 0, "tail");
    }
    const uint64_t total_bits = 8 * (digest_prefix + (uint64_t)ct_len);
    for (int i = 0; i < 8; i++) { S.lenblk[i] = (uint8_t)((uint64_t)(8 * aad_len) >> (56 - 8 * i)); S.lenblk[8 + i] = (uint8_t)((uint64_t)(8 * ct_len) >> (56 - 8 * i)); S.bits[i] = (uint8_t)(total_bits >> (56 - 8 * i)); }
    return S;
}
std::vector<zk::Fr> gcm_digest_public_input(size_t s, const DgShape &S, size_t c, const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const uint8_t *ct, const uint8_t tag[16],
                                            const uint8_t *commitments, const uint8_t *states) {
    uint8_t hd[16];
    memcpy(hd, iv, 12);
    const uint32_t ctr0 = (uint32_t)(2 + s * c);
    for (int i = 0; i < 4; i++) hd[12 + i] = (uint8_t)(ctr0 >> (24 - 8 * i));
    const bool first = s == 0, data = s < S.nd, fin = s + 1 == S.nd;
    return zk::public_input_of({{hd, 16}, {first ? aad : nullptr, aad_len}, {data ? ct + 16 * c * s : nullptr, fin ? S.lr : 16 * c}, {data ? nullptr : S.lenblk, 16}, {data ? nullptr : tag, 16},
                                {first ? nullptr : commitments + 32 * (s - 1), 32}, {data ? commitments + 32 * s : nullptr, 32}, {data ? states + 32 * s : nullptr, 64},
                                {fin ? S.bits : nullptr, 8}});
}
// ---- VK transport, library-private layout v2: "ZVK2", num_public_inputs (u64 LE), then the ark-serialize compressed image (marlin_codec.cpp).  Round 5's v1 was a memory
// image of the struct: reading it back from untrusted bytes put arbitrary limbs into field elements and an arbitrary byte into a bool, and skipped the curve / subgroup
// checks the ark path makes -- found while writing the fuzz target (tests/fuzz_host.cpp).  v2 goes through deserialize_vk_ark and inherits every check.
constexpr uint8_t VK_MAGIC[4] = {'Z', 'V', 'K', '2'};
}  // namespace
namespace zk { void capi_set_error(const std::string &m) { g_err = m; } }
namespace { thread_local zk::BatchTimings g_batch_timings; }
namespace zk { namespace capi { void set_last_batch_timings(const BatchTimings &t) { g_batch_timings = t; } } }
// The segment-proofs of one record through ONE multi-key batch: the checks of verify_gcm_segments, the rows of gcm_segment_public_input, head, mid and
// tail as keys 0, 1 and 2 of verify_batch_keys (a record of two segments has no mid: its tail is key 1).  mask = NULL: plain keys
void zk::capi::verify_gcm_segments_batch_call(const char *entry, const zkaes_vk *head, const zkaes_vk *mid_or_null, const zkaes_vk *tail, const uint8_t *proofs, const size_t *proof_lens,
                                              size_t n_segments, size_t c, const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const uint8_t *ct, size_t ct_len, const uint8_t tag[16],
                                              const uint8_t *commitments, size_t commitments_len, const uint8_t *mask, size_t mask_len, const uint8_t *revealed, size_t revealed_len,
                                              int *accepted_each, size_t *n_accepted, BatchBackend &be, const uint8_t *key_tag, size_t key_tag_len) {
    if (n_accepted) *n_accepted = 0;
    if (accepted_each) for (size_t s = 0; s < n_segments; s++) accepted_each[s] = 0;
    if (!proofs || !proof_lens) throw std::invalid_argument("null argument");
    const bool reveal = mask != nullptr;
    const SegShape S = gcm_segments_shape(entry, true, head, mid_or_null, tail, n_segments, c, iv, aad, aad_len, ct, ct_len, tag, commitments, commitments_len, reveal, mask, mask_len, revealed,
                                          revealed_len, key_tag, key_tag_len);
    std::vector<uint8_t> bits;
    std::vector<size_t> lens;
    std::vector<int> roles;
    gcm_segment_rows(S, c, iv, aad, aad_len, ct, tag, commitments, mask, revealed, &bits, lens, roles, key_tag, key_tag_len);      // (a head row that does not pad to its key's |X| is rejected alone)
    const zkaes_vk *vks[3] = {head, S.n > 2 ? mid_or_null : tail, tail};
    const size_t n_keys = S.n > 2 ? 3 : 2;
    std::vector<uint32_t> key_of(S.n);
    for (size_t s = 0; s < S.n; s++) key_of[s] = s == 0 ? 0 : (uint32_t)(s + 1 == S.n ? n_keys - 1 : 1);
    verify_batch_keys_call(vks, n_keys, key_of.data(), proofs, proof_lens, S.n, bits.data(), lens.data(), accepted_each, n_accepted, be);
}
using zk::capi::guard; using zk::capi::give; using zk::capi::fill_info; using zk::capi::next_pow2;

extern "C" {

const char *zkaes_last_error(void) { return g_err.c_str(); }
void zkaes_bytes_free(uint8_t *p) { free(p); }
void zkaes_vk_free(zkaes_vk *vk) { delete vk; }

int zkaes_verify(const zkaes_vk *vk, const uint8_t *proof, size_t proof_len, const uint8_t *bits, size_t n_bits, int *accepted) {
    return guard([&] {
        if (!vk || !proof || !accepted) throw std::invalid_argument("null argument");
        zk::Proof p = zk::deserialize_proof(proof, proof_len);
        std::vector<zk::Fr> pub(n_bits);
        for (size_t i = 0; i < n_bits; i++) pub[i] = bits[i] ? zk::Fr::one() : zk::Fr::zero();
        *accepted = zk::verify(vk->vk, pub, p) ? 1 : 0;
    });
}
int zkaes_verify_encryption(const zkaes_vk *vk, const uint8_t *proof, size_t proof_len, const uint8_t *ct, size_t ct_len, int *accepted) {
    return guard([&] {
        if (!vk || !proof || !accepted) throw std::invalid_argument("null argument");
        zk::Proof p = zk::deserialize_proof(proof, proof_len);
        *accepted = zk::verify(vk->vk, zk::ciphertext_to_public_input(ct, ct_len), p) ? 1 : 0;
    });
}
int zkaes_cbc_ciphertext(const uint8_t *msg, size_t len, const uint8_t key[16], const uint8_t iv[16], uint8_t *ct) {
    return guard([&] {
        if (!msg || !key || !iv || !ct) throw std::invalid_argument("null argument");
        if (len == 0 || len % 16) throw std::invalid_argument("CBC: the message must be a non-zero multiple of 16 bytes");
        zk::aes128_cbc_encrypt_host(msg, len, key, iv, ct);
    });
}
int zkaes_ecb_ciphertext_ks(const uint8_t *msg, size_t len, const uint8_t *key, size_t key_len, uint8_t *ct) {
    return guard([&] {
        if (!msg || !key || !ct) throw std::invalid_argument("null argument");
        require_key_len(key_len);
        if (len == 0 || len % 16) throw std::invalid_argument("ECB: the message must be a non-zero multiple of 16 bytes");
        zk::aes_ecb_encrypt_host(msg, len, key, key_len, ct);
    });
}
int zkaes_cbc_ciphertext_ks(const uint8_t *msg, size_t len, const uint8_t *key, size_t key_len, const uint8_t iv[16], uint8_t *ct) {
    return guard([&] {
        if (!msg || !key || !iv || !ct) throw std::invalid_argument("null argument");
        require_key_len(key_len);
        if (len == 0 || len % 16) throw std::invalid_argument("CBC: the message must be a non-zero multiple of 16 bytes");
        zk::aes128_cbc_encrypt_host(msg, len, key, iv, ct, key_len);
    });
}
int zkaes_verify_encryption_cbc(const zkaes_vk *vk, const uint8_t *proof, size_t proof_len, const uint8_t iv[16], const uint8_t *ct, size_t ct_len, int *accepted) {
    return guard([&] {
        if (!vk || !proof || !iv || !ct || !accepted) throw std::invalid_argument("null argument");
        *accepted = 0;
        if (ct_len == 0 || ct_len % 16) throw std::invalid_argument("CBC: the ciphertext must be a non-zero multiple of 16 bytes");
        zk::Proof p = zk::deserialize_proof(proof, proof_len);
        *accepted = zk::verify(vk->vk, zk::public_input_of({{iv, 16}, {ct, ct_len}}), p) ? 1 : 0;
    });
}
// Chunk j is checked against (IV_j, its slice of the ciphertext), IV_0 = iv and IV_j = the 16 ciphertext bytes ahead of the slice: all of it public, so the
// chunks are independent statements.  A chunk whose proof bytes do not parse is a rejected chunk, not an error of the call.
int zkaes_verify_cbc_chunked(const zkaes_vk *vk, const uint8_t *proofs, const size_t *proof_lens, size_t n_chunks, const uint8_t iv[16], const uint8_t *ct, size_t ct_len,
                             int *accepted_each, size_t *n_accepted) {
    return guard([&] {
        if (!vk || !proofs || !proof_lens || !iv || !ct) throw std::invalid_argument("null argument");
        if (n_accepted) *n_accepted = 0;
        if (n_chunks == 0 || ct_len == 0 || ct_len % n_chunks || (ct_len / n_chunks) % 16) throw std::invalid_argument("CBC: the ciphertext must be n_chunks x a non-zero multiple of 16 bytes");
        verify_chunks(vk->vk, zk::CIRCUIT_AES_CBC, proofs, proof_lens, n_chunks, ct_len / n_chunks, iv, ct, nullptr, 0, nullptr, accepted_each, n_accepted);
    });
}
// ---- AES-128-CTR.  The public input has the shape of CBC's: 128 bits of the initial counter block, then the ciphertext bits.
int zkaes_ctr_crypt(const uint8_t *in, size_t len, const uint8_t key[16], const uint8_t icb[16], uint8_t *out) {
    return guard([&] {
        if (!in || !key || !icb || !out) throw std::invalid_argument("null argument");
        if (len == 0) throw std::invalid_argument("CTR: the message must have at least one byte");
        zk::aes128_ctr_crypt_host(in, len, key, icb, out);
    });
}
int zkaes_ctr_crypt_ks(const uint8_t *in, size_t len, const uint8_t *key, size_t key_len, const uint8_t icb[16], uint8_t *out) {
    return guard([&] {
        if (!in || !key || !icb || !out) throw std::invalid_argument("null argument");
        require_key_len(key_len);
        if (len == 0) throw std::invalid_argument("CTR: the message must have at least one byte");
        zk::aes128_ctr_crypt_host(in, len, key, icb, out, key_len);
    });
}
int zkaes_ctr_counter_add(const uint8_t icb[16], uint64_t n_blocks, uint8_t out[16]) {
    return guard([&] {
        if (!icb || !out) throw std::invalid_argument("null argument");
        zk::ctr_counter_add(icb, n_blocks, out);
    });
}
namespace {
// The verifier zero-pads the public input to |X| - 1, so a ciphertext with zero bytes appended would give the same padded vector: the byte length is part of the
// statement and is checked against the key's own count.  A key that came through the ark transport carries only the padded count (marlin_codec.cpp); for such a key the
// length is checked as far as |X| tells (zk::verify rejects another |X|) and the caller answers for the exact length.
void require_ctr_length(const zk::VerifyingKey &vk, size_t ct_len) {
    if (ct_len == 0) throw std::invalid_argument("CTR: the ciphertext must have at least one byte");
    bool exact = vk.num_public_inputs + 1 != vk.num_instance;
    if (exact && vk.num_public_inputs != 128 + 8 * ct_len) throw std::invalid_argument("CTR: the ciphertext length is not the one this key was synthesized for");
}
}  // namespace
int zkaes_verify_encryption_ctr(const zkaes_vk *vk, const uint8_t *proof, size_t proof_len, const uint8_t icb[16], const uint8_t *ct, size_t ct_len, int *accepted) {
    return guard([&] {
        if (!vk || !proof || !icb || !ct || !accepted) throw std::invalid_argument("null argument");
        *accepted = 0;
        require_ctr_length(vk->vk, ct_len);
        zk::Proof p = zk::deserialize_proof(proof, proof_len);
        *accepted = zk::verify(vk->vk, zk::public_input_of({{icb, 16}, {ct, ct_len}}), p) ? 1 : 0;
    });
}
// Chunk j is checked against (icb + j nb, its slice of the ciphertext), nb = the chunk's blocks: the counter comes from (icb, j) alone, so any chunk can be checked
// without the others.  A chunk whose proof bytes do not parse is a rejected chunk, not an error of the call.
int zkaes_verify_ctr_chunked(const zkaes_vk *vk, const uint8_t *proofs, const size_t *proof_lens, size_t n_chunks, const uint8_t icb[16], const uint8_t *ct, size_t ct_len,
                             int *accepted_each, size_t *n_accepted) {
    return guard([&] {
        if (!vk || !proofs || !proof_lens || !icb || !ct) throw std::invalid_argument("null argument");
        if (n_accepted) *n_accepted = 0;
        if (n_chunks == 0 || ct_len == 0 || ct_len % n_chunks || (ct_len / n_chunks) % 16) throw std::invalid_argument("CTR: the ciphertext must be n_chunks x a non-zero multiple of 16 bytes");
        const size_t chunk = ct_len / n_chunks;
        require_ctr_length(vk->vk, chunk);
        verify_chunks(vk->vk, zk::CIRCUIT_AES_CTR, proofs, proof_lens, n_chunks, chunk, icb, ct, nullptr, 0, nullptr, accepted_each, n_accepted);
    });
}
// ---- AES-128-GCM.  Public input: 96 iv bits, the aad bits, the ciphertext bits, 128 tag bits.
int zkaes_gcm_encrypt_ks(const uint8_t *msg, size_t len, const uint8_t *key, size_t key_len, const uint8_t iv[12], const uint8_t *aad, size_t aad_len, uint8_t *ct, uint8_t tag[16]) {
    return guard([&] {
        if (!key || !iv || !tag || (len && (!msg || !ct)) || (aad_len && !aad)) throw std::invalid_argument("null argument");
        require_key_len(key_len);
        zk::aes128_gcm_encrypt_host(msg, len, key, iv, aad, aad_len, ct, tag, key_len);
    });
}
int zkaes_gcm_encrypt(const uint8_t *msg, size_t len, const uint8_t key[16], const uint8_t iv[12], const uint8_t *aad, size_t aad_len, uint8_t *ct, uint8_t tag[16]) {
    return zkaes_gcm_encrypt_ks(msg, len, key, 16, iv, aad, aad_len, ct, tag);
}
int zkaes_gcm_decrypt(const uint8_t *ct, size_t len, const uint8_t key[16], const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const uint8_t tag[16], uint8_t *msg, int *ok) {
    return zkaes_gcm_decrypt_ks(ct, len, key, 16, iv, aad, aad_len, tag, msg, ok);
}
int zkaes_gcm_decrypt_ks(const uint8_t *ct, size_t len, const uint8_t *key, size_t key_len, const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const uint8_t tag[16], uint8_t *msg, int *ok) {
    return guard([&] {
        if (!key || !iv || !tag || !ok || (len && (!msg || !ct)) || (aad_len && !aad)) throw std::invalid_argument("null argument");
        *ok = 0;
        require_key_len(key_len);
        // GCM's keystream does not depend on the data, so "encrypting" the ciphertext gives the plaintext -- and a tag over that plaintext, not the one wanted: the tag is
        // GHASH over the CIPHERTEXT, which a second pass computes by encrypting the candidate plaintext back.  Nothing reaches the caller's buffer before the tag holds.
        std::vector<uint8_t> pt(len ? len : 1), back(len ? len : 1);
        uint8_t t[16];
        zk::aes128_gcm_encrypt_host(ct, len, key, iv, aad, aad_len, pt.data(), t, key_len);
        zk::aes128_gcm_encrypt_host(pt.data(), len, key, iv, aad, aad_len, back.data(), t, key_len);
        unsigned diff = 0;
        for (int i = 0; i < 16; i++) diff |= (unsigned)(t[i] ^ tag[i]);                // no early exit: the time does not tell where the tags differ
        if (diff) return;
        if (len) memcpy(msg, pt.data(), len);
        *ok = 1;
    });
}
namespace {
// the verifier zero-pads the public input, so the byte lengths are part of the statement (as require_ctr_length); the key pins A + L, and the length block inside its
// circuit pins the split between the two
void require_gcm_lengths(const zk::VerifyingKey &vk, size_t aad_len, size_t ct_len) {
    if (ct_len == 0) throw std::invalid_argument("GCM: the ciphertext must have at least one byte");
    bool exact = vk.num_public_inputs + 1 != vk.num_instance;
    if (exact && vk.num_public_inputs != 224 + 8 * (aad_len + ct_len)) throw std::invalid_argument("GCM: aad and ciphertext lengths are not the ones this key was synthesized for");
}
}  // namespace
int zkaes_verify_encryption_gcm(const zkaes_vk *vk, const uint8_t *proof, size_t proof_len, const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const uint8_t *ct, size_t ct_len,
                                const uint8_t tag[16], int *accepted) {
    return guard([&] {
        if (!vk || !proof || !iv || !ct || !tag || !accepted || (aad_len && !aad)) throw std::invalid_argument("null argument");
        *accepted = 0;
        require_gcm_lengths(vk->vk, aad_len, ct_len);
        zk::Proof p = zk::deserialize_proof(proof, proof_len);
        *accepted = zk::verify(vk->vk, gcm_public_input(iv, aad, aad_len, ct, ct_len, tag, nullptr, 0, nullptr, nullptr), p) ? 1 : 0;
    });
}
// ---- GCM segments (include/zkaes.h): Y at the boundaries and a commitment on the host, and the verifier of a record's n segment-proofs
int zkaes_gcm_boundaries(const uint8_t *msg, size_t len, const uint8_t *key, size_t key_len, const uint8_t iv[12], const uint8_t *aad, size_t aad_len, size_t c, uint8_t *ys, size_t ys_cap,
                         size_t *n_segments) {
    return guard([&] {
        if (!msg || !key || !iv || (aad_len && !aad)) throw std::invalid_argument("null argument");
        require_key_len(key_len);
        if (len == 0 || len > ((size_t)1 << 20) || c == 0) throw std::invalid_argument("GCM segments: a record has 1 .. 2^20 bytes and a segment at least one block");
        const size_t nb = (len + 15) / 16, n = (nb + c - 1) / c;
        if (n_segments) *n_segments = n;
        if (!ys) return;
        if (ys_cap < 16 * (n - 1)) throw std::invalid_argument("ys buffer too small: 16 bytes per boundary");
        zk::gcm_boundaries_host(msg, len, key, key_len, iv, aad, aad_len, c, ys);
    });
}
int zkaes_gcm_commit(const uint8_t *key, size_t key_len, const uint8_t y[16], const uint8_t salt[16], uint8_t com[32]) {
    return guard([&] {
        if (!key || !y || !salt || !com) throw std::invalid_argument("null argument");
        require_key_len(key_len);
        zk::gcm_commit_host(key, key_len, y, salt, com);
    });
}
// Segment s is checked against (iv, ctr0 = 2 + s c, its slice of the ciphertext) and its role's further inputs: the aad and commitments[0] (head), commitments[s - 1]
// and commitments[s] (mid), the length block built from the aad and ciphertext lengths seen HERE, the tag and commitments[n - 2] (tail).  One array of n - 1 commitments
// serves both sides of every boundary.  A segment whose proof bytes do not parse is a rejected segment, not an error of the call.
// With a mask (the _reveal entry) every segment's input ends in its slice of the record's ONE mask and of its revealed bytes, as a chunk's does
// (chunk_public_input): head, mid and tail together state revealed[i] = mask_i ? M[i] : 0 over the whole record.  The two entries refuse each other's keys: where a key
// carries its exact public-input count a proof of the other kind raises, otherwise it is rejected (its |X| or its index commitments differ)
int zkaes_verify_gcm_segments(const zkaes_vk *head, const zkaes_vk *mid_or_null, const zkaes_vk *tail, const uint8_t *proofs, const size_t *proof_lens, size_t n_segments, size_t c,
                              const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const uint8_t *ct, size_t ct_len, const uint8_t tag[16], const uint8_t *commitments, size_t commitments_len,
                              int *accepted_each, size_t *n_accepted) {
    return guard([&] {
        verify_gcm_segments("verify_gcm_segments", head, mid_or_null, tail, proofs, proof_lens, n_segments, c, iv, aad, aad_len, ct, ct_len, tag, commitments, commitments_len, false, nullptr, 0,
                            nullptr, 0, accepted_each, n_accepted);
    });
}
int zkaes_verify_gcm_segments_reveal(const zkaes_vk *head, const zkaes_vk *mid_or_null, const zkaes_vk *tail, const uint8_t *proofs, const size_t *proof_lens, size_t n_segments, size_t c,
                                     const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const uint8_t *ct, size_t ct_len, const uint8_t tag[16], const uint8_t *commitments,
                                     size_t commitments_len, const uint8_t *mask, size_t mask_len, const uint8_t *revealed, size_t revealed_len, int *accepted_each, size_t *n_accepted) {
    return guard([&] {
        verify_gcm_segments("verify_gcm_segments_reveal", head, mid_or_null, tail, proofs, proof_lens, n_segments, c, iv, aad, aad_len, ct, ct_len, tag, commitments, commitments_len, true, mask,
                            mask_len, revealed, revealed_len, accepted_each, n_accepted);
    });
}
// ---- key tags (include/zkaes.h): the tag on the host, and the verifiers that check every proof of a job against ONE tag
int zkaes_key_tag(const uint8_t *secret_key, size_t key_len, size_t tag_blocks, uint8_t *out) {
    return guard([&] {
        if (!secret_key || !out) throw std::invalid_argument("null argument");
        require_key_len(key_len);
        zk::aes_key_tag_host(secret_key, key_len, tag_blocks, out);
    });
}
namespace {
void require_key_tag_len(size_t key_tag_len) { if (key_tag_len != 16 && key_tag_len != 32) throw std::invalid_argument("key_tag_len must be 16 or 32 (one or two tag blocks)"); }
// Does a public input of n_bits bits fit this key?  Where the key carries its exact count a mismatch raises (the verifier zero-pads, so a wrong tag length must never
// reach it); a key from the ark transport carries only |X|, so there the answer is "rejected" unless the padded counts agree, and the caller answers for the rest
bool fits_key(const zk::VerifyingKey &vk, size_t n_bits, const char *what) {
    bool exact = vk.num_public_inputs + 1 != vk.num_instance;
    if (exact && vk.num_public_inputs != n_bits) throw std::invalid_argument(std::string(what) + ": the ciphertext and key-tag lengths are not the ones this key was synthesized for");
    return next_pow2(n_bits + 1) == vk.num_instance;
}
void require_opt_key_tag(const uint8_t *key_tag, size_t key_tag_len) {
    if (key_tag ? (key_tag_len != 16 && key_tag_len != 32) : key_tag_len != 0) throw std::invalid_argument("key_tag_len must be 16 or 32 with a key tag, 0 with NULL");
}
// The shape of a chunked ECB, CBC or CTR job as zkaes_verify_chunked_kt, zkaes_verify_digest_chunked and zkaes_chunk_public_inputs take it -> the slice's byte length.
// `entry` opens every message; gcm_entry names where GCM records go instead (null: not said); a key tag is optional unless tag_required
size_t require_slices(const std::string &entry, const char *gcm_entry, int circuit_kind, const uint8_t *iv_or_icb, size_t n_chunks, size_t ct_len, const uint8_t *key_tag, size_t key_tag_len,
                      bool tag_required) {
    const bool ecb = circuit_kind == zk::CIRCUIT_AES, cbc = circuit_kind == zk::CIRCUIT_AES_CBC, ctr = circuit_kind == zk::CIRCUIT_AES_CTR;
    if (!ecb && !cbc && !ctr) throw std::invalid_argument(entry + ": circuit_kind must be ECB, CBC or CTR" + (gcm_entry ? std::string(" (GCM records go through ") + gcm_entry + ")" : std::string()));
    if (ecb ? iv_or_icb != nullptr : iv_or_icb == nullptr) throw std::invalid_argument(entry + ": an iv or initial counter block for CBC and CTR, NULL for ECB");
    if (tag_required) require_key_tag_len(key_tag_len); else require_opt_key_tag(key_tag, key_tag_len);
    if (n_chunks == 0 || ct_len == 0 || ct_len % n_chunks) throw std::invalid_argument(entry + ": the ciphertext must be n_chunks equal, non-empty slices");
    const size_t chunk = ct_len / n_chunks;
    if (chunk % 16 && !(ctr && n_chunks == 1)) throw std::invalid_argument(entry + ": every slice must be whole blocks (a lone CTR proof takes any length)");
    return chunk;
}
}  // namespace
// Chunk j's public input is what zkaes_verify_encryption (ECB), zkaes_verify_cbc_chunked or zkaes_verify_ctr_chunked derive for it, with the tag bits appended.  n_chunks = 1
// is the lone-proof form, and the only one that takes a CTR ciphertext that is not whole blocks
int zkaes_verify_chunked_kt(const zkaes_vk *vk, int circuit_kind, const uint8_t *proofs, const size_t *proof_lens, size_t n_chunks, const uint8_t *iv_or_icb, const uint8_t *ct, size_t ct_len,
                            const uint8_t *key_tag, size_t key_tag_len, int *accepted_each, size_t *n_accepted) {
    return guard([&] {
        if (n_accepted) *n_accepted = 0;
        if (accepted_each) for (size_t j = 0; j < n_chunks; j++) accepted_each[j] = 0;
        if (!vk || !proofs || !proof_lens || !ct || !key_tag) throw std::invalid_argument("null argument");
        const size_t chunk = require_slices("verify_chunked_kt", "zkaes_verify_encryption_gcm_kt", circuit_kind, iv_or_icb, n_chunks, ct_len, key_tag, key_tag_len, true);
        if (!fits_key(vk->vk, (iv_or_icb ? 128 : 0) + 8 * chunk + 8 * key_tag_len, "verify_chunked_kt")) return;      // every chunk rejected
        verify_chunks(vk->vk, circuit_kind, proofs, proof_lens, n_chunks, chunk, iv_or_icb, ct, key_tag, key_tag_len, nullptr, accepted_each, n_accepted);
    });
}
int zkaes_verify_encryption_gcm_kt(const zkaes_vk *vk, const uint8_t *proof, size_t proof_len, const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const uint8_t *ct, size_t ct_len,
                                   const uint8_t tag[16], const uint8_t *key_tag, size_t key_tag_len, int *accepted) {
    return guard([&] {
        if (accepted) *accepted = 0;
        if (!vk || !proof || !iv || !ct || !tag || !key_tag || !accepted || (aad_len && !aad)) throw std::invalid_argument("null argument");
        require_key_tag_len(key_tag_len);
        if (ct_len == 0) throw std::invalid_argument("GCM: the ciphertext must have at least one byte");
        if (!fits_key(vk->vk, 224 + 8 * (aad_len + ct_len) + 8 * key_tag_len, "GCM")) return;
        zk::Proof p = zk::deserialize_proof(proof, proof_len);
        *accepted = zk::verify(vk->vk, gcm_public_input(iv, aad, aad_len, ct, ct_len, tag, key_tag, key_tag_len, nullptr, nullptr), p) ? 1 : 0;
    });
}
// ---- plaintext digests (include/zkaes.h): SHA-256 on the host, and the verifiers that check every proof of a job against ONE array of states
int zkaes_sha256_chain(const uint8_t *h_in, const uint8_t *data, size_t len, uint8_t h_out[32]) {
    return guard([&] {
        if (!h_out || (!data && len)) throw std::invalid_argument("null argument");
        zk::sha256_chain(h_in, data, len, h_out);
    });
}
int zkaes_sha256_finish(const uint8_t *h_in, uint64_t prefix_bytes, const uint8_t *tail, size_t tail_len, uint8_t digest[32]) {
    return guard([&] {
        if (!digest || (!tail && tail_len)) throw std::invalid_argument("null argument");
        zk::sha256_finish(h_in, prefix_bytes, tail, tail_len, digest);
    });
}
int zkaes_verify_digest_chunked(const zkaes_vk *vk, int circuit_kind, const uint8_t *proofs, const size_t *proof_lens, size_t n_chunks, const uint8_t *iv_or_icb, const uint8_t *ct, size_t ct_len,
                                const uint8_t *key_tag, size_t key_tag_len, const uint8_t *states, int *accepted_each, size_t *n_accepted) {
    return guard([&] {
        if (n_accepted) *n_accepted = 0;
        if (accepted_each) for (size_t j = 0; j < n_chunks; j++) accepted_each[j] = 0;
        if (!vk || !proofs || !proof_lens || !ct || !states) throw std::invalid_argument("null argument");
        const size_t chunk = require_slices("verify_digest_chunked", "zkaes_verify_encryption_gcm_digest", circuit_kind, iv_or_icb, n_chunks, ct_len, key_tag, key_tag_len, false);
        if (!fits_key(vk->vk, (iv_or_icb ? 128 : 0) + 8 * chunk + 8 * key_tag_len + 512, "verify_digest_chunked")) return;      // every chunk rejected
        verify_chunks(vk->vk, circuit_kind, proofs, proof_lens, n_chunks, chunk, iv_or_icb, ct, key_tag, key_tag_len, states, accepted_each, n_accepted);
    });
}
int zkaes_verify_encryption_gcm_digest(const zkaes_vk *vk, const uint8_t *proof, size_t proof_len, const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const uint8_t *ct, size_t ct_len,
                                       const uint8_t tag[16], const uint8_t *key_tag, size_t key_tag_len, const uint8_t *h_in, const uint8_t h_out[32], int *accepted) {
    return guard([&] {
        if (accepted) *accepted = 0;
        if (!vk || !proof || !iv || !ct || !tag || !h_out || !accepted || (aad_len && !aad)) throw std::invalid_argument("null argument");
        require_opt_key_tag(key_tag, key_tag_len);
        if (ct_len == 0) throw std::invalid_argument("GCM: the ciphertext must have at least one byte");
        if (!fits_key(vk->vk, 224 + 8 * (aad_len + ct_len) + 8 * key_tag_len + 512, "GCM")) return;
        zk::Proof p = zk::deserialize_proof(proof, proof_len);
        uint8_t iv0[32];
        zk::sha256_chain(nullptr, nullptr, 0, iv0);
        *accepted = zk::verify(vk->vk, gcm_public_input(iv, aad, aad_len, ct, ct_len, tag, key_tag, key_tag_len, h_in ? h_in : iv0, h_out), p) ? 1 : 0;
    });
}
// ---- selective disclosure (include/zkaes.h): the masking on the host, and the verifiers that check every proof of a job against ONE mask and ONE array of
// revealed bytes.  A mask bit at or beyond the length, or a non-zero revealed byte under a zero mask bit, is an ERROR of the call (statement.hpp), never a rejection
int zkaes_reveal_bytes(const uint8_t *msg, size_t len, const uint8_t *mask, size_t mask_len, uint8_t *out) {
    return guard([&] {
        if ((len && (!msg || !out)) || !mask) throw std::invalid_argument("null argument");
        if (mask_len != zk::mask_bytes(len)) throw std::invalid_argument("reveal_bytes: a mask over " + std::to_string(len) + " bytes has " + std::to_string(zk::mask_bytes(len)) + " bytes");
        zk::require_mask(mask, len);
        zk::reveal_bytes(msg, mask, len, out);
    });
}
int zkaes_verify_reveal_chunked(const zkaes_vk *vk, int circuit_kind, const uint8_t *proofs, const size_t *proof_lens, size_t n_chunks, const uint8_t *iv_or_icb, const uint8_t *ct, size_t ct_len,
                                const uint8_t *key_tag, size_t key_tag_len, const uint8_t *states, const uint8_t *mask, size_t mask_len, const uint8_t *revealed, int *accepted_each,
                                size_t *n_accepted) {
    return guard([&] {
        if (n_accepted) *n_accepted = 0;
        if (accepted_each) for (size_t j = 0; j < n_chunks; j++) accepted_each[j] = 0;
        if (!vk || !proofs || !proof_lens || !ct || !mask || !revealed) throw std::invalid_argument("null argument");
        const size_t chunk = require_slices("verify_reveal_chunked", "zkaes_verify_encryption_gcm_reveal", circuit_kind, iv_or_icb, n_chunks, ct_len, key_tag, key_tag_len, false);
        if (mask_len != zk::mask_bytes(ct_len)) throw std::invalid_argument("verify_reveal_chunked: ONE mask over the whole job, " + std::to_string(zk::mask_bytes(ct_len)) + " bytes for this ciphertext");
        zk::require_revealed(mask, revealed, ct_len);
        if (!fits_key(vk->vk, (iv_or_icb ? 128 : 0) + 8 * chunk + 8 * key_tag_len + (states ? 512 : 0) + 8 * zk::mask_bytes(chunk) + 8 * chunk, "verify_reveal_chunked")) return;      // every chunk rejected
        verify_chunks(vk->vk, circuit_kind, proofs, proof_lens, n_chunks, chunk, iv_or_icb, ct, key_tag, key_tag_len, states, accepted_each, n_accepted, mask, revealed);
    });
}
int zkaes_verify_encryption_gcm_reveal(const zkaes_vk *vk, const uint8_t *proof, size_t proof_len, const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const uint8_t *ct, size_t ct_len,
                                       const uint8_t tag[16], const uint8_t *key_tag, size_t key_tag_len, const uint8_t *h_in, const uint8_t *h_out, const uint8_t *mask, size_t mask_len,
                                       const uint8_t *revealed, int *accepted) {
    return guard([&] {
        if (accepted) *accepted = 0;
        if (!vk || !proof || !iv || !ct || !tag || !mask || !revealed || !accepted || (aad_len && !aad) || (h_in && !h_out)) throw std::invalid_argument("null argument");
        require_opt_key_tag(key_tag, key_tag_len);
        if (ct_len == 0) throw std::invalid_argument("GCM: the ciphertext must have at least one byte");
        if (mask_len != zk::mask_bytes(ct_len)) throw std::invalid_argument("GCM: a mask over this ciphertext has " + std::to_string(zk::mask_bytes(ct_len)) + " bytes");
        zk::require_revealed(mask, revealed, ct_len);
        if (!fits_key(vk->vk, 224 + 8 * (aad_len + ct_len) + 8 * key_tag_len + (h_out ? 512 : 0) + 8 * mask_len + 8 * ct_len, "GCM")) return;
        zk::Proof p = zk::deserialize_proof(proof, proof_len);
        uint8_t iv0[32];
        zk::sha256_chain(nullptr, nullptr, 0, iv0);
        *accepted = zk::verify(vk->vk, gcm_public_input(iv, aad, aad_len, ct, ct_len, tag, key_tag, key_tag_len, h_out ? (h_in ? h_in : iv0) : nullptr, h_out, mask, revealed), p) ? 1 : 0;
    });
}
int zkaes_proof_roundtrip(const uint8_t *proof, size_t proof_len, uint8_t **out, size_t *out_len) {
    return guard([&] { auto b = zk::serialize_proof(zk::deserialize_proof(proof, proof_len)); *out = give(b); *out_len = b.size(); });
}
int zkaes_vk_serialize(const zkaes_vk *vk, uint8_t **out, size_t *out_len) {
    return guard([&] {
        if (!vk || !out || !out_len) throw std::invalid_argument("null argument");
        std::vector<uint8_t> b(VK_MAGIC, VK_MAGIC + 4);
        for (int i = 0; i < 8; i++) b.push_back((uint8_t)((uint64_t)vk->vk.num_public_inputs >> (8 * i)));
        auto ark = zk::serialize_vk_ark(vk->vk);
        b.insert(b.end(), ark.begin(), ark.end());
        *out = give(b); *out_len = b.size();
    });
}
int zkaes_vk_serialize_ark(const zkaes_vk *vk, uint8_t **out, size_t *out_len) {
    return guard([&] {
        if (!vk || !out || !out_len) throw std::invalid_argument("null argument");
        auto b = zk::serialize_vk_ark(vk->vk);
        *out = give(b); *out_len = b.size();
    });
}
int zkaes_vk_serialize_ark_uncompressed(const zkaes_vk *vk, uint8_t **out, size_t *out_len) {
    return guard([&] {
        if (!vk || !out || !out_len) throw std::invalid_argument("null argument");
        auto b = zk::serialize_vk_ark(vk->vk, true);
        *out = give(b); *out_len = b.size();
    });
}
int zkaes_vk_deserialize_ark(const uint8_t *bytes, size_t len, zkaes_vk **vk) {
    return guard([&] {
        if (!bytes || !vk) throw std::invalid_argument("null argument");
        *vk = new zkaes_vk{zk::deserialize_vk_ark(bytes, len)};
    });
}
int zkaes_vk_deserialize(const uint8_t *bytes, size_t len, zkaes_vk **vk) {
    return guard([&] {
        if (!bytes || !vk) throw std::invalid_argument("null argument");
        if (len < 12) throw std::runtime_error("vk_deserialize: truncated");
        if (memcmp(bytes, VK_MAGIC, 4) != 0) throw std::runtime_error("vk_deserialize: bad magic");
        uint64_t npub = 0;
        for (int i = 0; i < 8; i++) npub |= (uint64_t)bytes[4 + i] << (8 * i);
        std::unique_ptr<zkaes_vk> v(new zkaes_vk{zk::deserialize_vk_ark(bytes + 12, len - 12)});
        if (npub + 1 > v->vk.num_instance) throw std::runtime_error("vk_deserialize: more public inputs than instance variables");
        v->vk.num_public_inputs = (size_t)npub;
        *vk = v.release();
    });
}
int zkaes_vk_from_trapdoor(const uint64_t info[7], const uint8_t *index_comms, const uint8_t *beta_b, zkaes_vk **vk) {
    return guard([&] {
        if (!info || !index_comms || !beta_b || !vk) throw std::invalid_argument("null argument");
        zk::Fr beta_in, beta;
        memcpy(beta_in.l, beta_b, 32);
        zk::G1A g, gamma_g;
        zk::pairing::G2Affine h;
        zk::kzg_setup_points(beta, g, gamma_g, h);                   // this library's own replay of KZG10::setup's draws from test_rng
        if (!(beta == beta_in)) throw std::invalid_argument("vk_from_trapdoor: beta is not the first Fr draw of ark_std::test_rng()");
        zkaes_vk *v = new zkaes_vk();
        zk::VerifyingKey &k = v->vk;
        k.num_variables = info[0]; k.num_constraints = info[1]; k.num_non_zero = info[2]; k.num_instance = info[3];
        k.num_public_inputs = info[4]; k.max_degree = info[5]; k.supported_degree = info[6];
        for (int i = 0; i < 6; i++) { memcpy(k.index_comms[i].x.l, index_comms + 96 * i, 48); memcpy(k.index_comms[i].y.l, index_comms + 96 * i + 48, 48); }
        auto mulg = [&](const zk::Fr &s) { return zk::mul_fr(zk::XYZZ<zk::Fq377>::from_affine(g), s).to_affine(); };
        k.g = g; k.gamma_g = gamma_g; k.h = h;
        uint32_t raw[8]; beta.to_raw(raw);
        k.beta_h = zk::pairing::g2_mul_raw(k.h, raw, 8);
        size_t n = next_pow2(k.num_constraints), kk = next_pow2(k.num_non_zero);
        k.degree_bounds[0] = std::min(n - 2, kk - 2); k.degree_bounds[1] = std::max(n - 2, kk - 2);
        for (int i = 0; i < 2; i++) k.shift_powers[i] = mulg(beta.pow_u64(k.max_degree - k.degree_bounds[i]));
        *vk = v;
    });
}
int zkaes_circuit_info(int kind, size_t len, uint64_t out[12]) { return guard([&] { fill_info(compile(kind, len), out); }); }
int zkaes_circuit_info_gcm(size_t len, size_t aad_len, uint64_t out[12]) { return guard([&] { fill_info(compile(zk::CIRCUIT_AES_GCM, len, aad_len), out); }); }
int zkaes_circuit_info_ks(int kind, unsigned key_bits, size_t len, size_t aad_len, uint64_t out[12]) { return guard([&] { fill_info(compile(kind, len, aad_len, key_bits), out); }); }
int zkaes_circuit_info_kt(int kind, unsigned key_bits, unsigned key_tag_blocks, size_t len, size_t aad_len, uint64_t out[12]) {
    return guard([&] { fill_info(compile(kind, len, aad_len, key_bits, key_tag_blocks), out); });
}
int zkaes_circuit_info_pd(int kind, unsigned key_bits, unsigned key_tag_blocks, unsigned digest_kind, uint64_t digest_prefix, size_t len, size_t aad_len, uint64_t out[12]) {
    return guard([&] { fill_info(compile(kind, len, aad_len, key_bits, key_tag_blocks, (int)digest_kind, digest_prefix), out); });
}
int zkaes_circuit_info_rv(int kind, unsigned key_bits, unsigned key_tag_blocks, unsigned digest_kind, uint64_t digest_prefix, unsigned reveal, size_t len, size_t aad_len, uint64_t out[12]) {
    return guard([&] { fill_info(compile(kind, len, aad_len, key_bits, key_tag_blocks, (int)digest_kind, digest_prefix, reveal > 1 ? 2 : (int)reveal), out); });
}
static int circuit_matrix(int kind, size_t len, size_t aad_len, int which, uint64_t *n_rows, uint64_t *nnz, uint32_t *rowptr, uint32_t *col, int64_t *coeff, size_t key_bits = 128,
                          size_t key_tag_blocks = 0, int digest_kind = 0, uint64_t digest_prefix = 0, int reveal = 0) {
    return guard([&] {
        zk::Circuit c = compile(kind, len, aad_len, key_bits, key_tag_blocks, digest_kind, digest_prefix, reveal);
        const zk::CsrMatrix &m = which == 0 ? c.A : which == 1 ? c.B : c.C;
        if (n_rows) *n_rows = m.rows();
        if (nnz) *nnz = m.nnz();
        if (rowptr) memcpy(rowptr, m.rowptr.data(), m.rowptr.size() * 4);
        if (col) memcpy(col, m.col.data(), m.col.size() * 4);
        if (coeff) memcpy(coeff, m.coeff.data(), m.coeff.size() * 8);
    });
}
int zkaes_circuit_matrix(int kind, size_t len, int which, uint64_t *n_rows, uint64_t *nnz, uint32_t *rowptr, uint32_t *col, int64_t *coeff) {
    return circuit_matrix(kind, len, 0, which, n_rows, nnz, rowptr, col, coeff);
}
int zkaes_circuit_matrix_ks(int kind, unsigned key_bits, size_t len, size_t aad_len, int which, uint64_t *n_rows, uint64_t *nnz, uint32_t *rowptr, uint32_t *col, int64_t *coeff) {
    return circuit_matrix(kind, len, aad_len, which, n_rows, nnz, rowptr, col, coeff, key_bits);
}
int zkaes_circuit_matrix_kt(int kind, unsigned key_bits, unsigned key_tag_blocks, size_t len, size_t aad_len, int which, uint64_t *n_rows, uint64_t *nnz, uint32_t *rowptr, uint32_t *col,
                            int64_t *coeff) {
    return circuit_matrix(kind, len, aad_len, which, n_rows, nnz, rowptr, col, coeff, key_bits, key_tag_blocks);
}
int zkaes_circuit_matrix_pd(int kind, unsigned key_bits, unsigned key_tag_blocks, unsigned digest_kind, uint64_t digest_prefix, size_t len, size_t aad_len, int which, uint64_t *n_rows,
                            uint64_t *nnz, uint32_t *rowptr, uint32_t *col, int64_t *coeff) {
    return circuit_matrix(kind, len, aad_len, which, n_rows, nnz, rowptr, col, coeff, key_bits, key_tag_blocks, (int)digest_kind, digest_prefix);
}
int zkaes_circuit_matrix_rv(int kind, unsigned key_bits, unsigned key_tag_blocks, unsigned digest_kind, uint64_t digest_prefix, unsigned reveal, size_t len, size_t aad_len, int which,
                            uint64_t *n_rows, uint64_t *nnz, uint32_t *rowptr, uint32_t *col, int64_t *coeff) {
    return circuit_matrix(kind, len, aad_len, which, n_rows, nnz, rowptr, col, coeff, key_bits, key_tag_blocks, (int)digest_kind, digest_prefix, reveal > 1 ? 2 : (int)reveal);
}
int zkaes_circuit_matrix_gcm(size_t len, size_t aad_len, int which, uint64_t *n_rows, uint64_t *nnz, uint32_t *rowptr, uint32_t *col, int64_t *coeff) {
    return circuit_matrix(zk::CIRCUIT_AES_GCM, len, aad_len, which, n_rows, nnz, rowptr, col, coeff);
}
// (this query also fills out[9 .. 11]: the non-zeros of the joint matrix -- the positions where A, B or C has an entry, as the indexer merges them -- and |H|, |K|, so
// that a caller can size a record's segments against an SRS without a device)
static int circuit_info_gcm_seg(int role, unsigned key_bits, size_t units, size_t aad_len, unsigned reveal, unsigned key_tag_blocks, uint64_t out[12], int digest = 0) {
    return guard([&] {
        const zk::Circuit c = zk::compile_aes_gcm_segment_circuit(role, units, aad_len, key_bits, reveal > 1 ? 2 : (int)reveal, key_tag_blocks, digest);
        fill_info(c, out);
        uint64_t joint = 0;
        for (size_t r = 0; r < c.num_constraints; r++) {
            uint32_t ia = c.A.rowptr[r], ib = c.B.rowptr[r], ic = c.C.rowptr[r];
            const uint32_t ea = c.A.rowptr[r + 1], eb = c.B.rowptr[r + 1], ec = c.C.rowptr[r + 1];
            for (;;) {                                                                   // the per-row sorted union of the three column supports
                uint32_t best = 0xffffffffu;
                if (ia < ea) best = std::min(best, c.A.col[ia]);
                if (ib < eb) best = std::min(best, c.B.col[ib]);
                if (ic < ec) best = std::min(best, c.C.col[ic]);
                if (best == 0xffffffffu) break;
                joint++;
                if (ia < ea && c.A.col[ia] == best) ia++;
                if (ib < eb && c.B.col[ib] == best) ib++;
                if (ic < ec && c.C.col[ic] == best) ic++;
            }
        }
        out[9] = joint; out[10] = next_pow2(c.num_constraints); out[11] = next_pow2(joint);
    });
}
int zkaes_circuit_info_gcm_seg(int role, unsigned key_bits, size_t units, size_t aad_len, uint64_t out[12]) { return circuit_info_gcm_seg(role, key_bits, units, aad_len, 0, 0, out); }
int zkaes_circuit_info_gcm_seg_rv(int role, unsigned key_bits, unsigned reveal, size_t units, size_t aad_len, uint64_t out[12]) { return circuit_info_gcm_seg(role, key_bits, units, aad_len, reveal, 0, out); }
int zkaes_circuit_info_gcm_seg_kt(int role, unsigned key_bits, unsigned reveal, unsigned key_tag_blocks, size_t units, size_t aad_len, uint64_t out[12]) {
    return circuit_info_gcm_seg(role, key_bits, units, aad_len, reveal, key_tag_blocks, out);
}
int zkaes_circuit_info_gcm_seg_dg(int role, unsigned key_bits, size_t units, size_t aad_len, uint64_t out[12]) { return circuit_info_gcm_seg(role, key_bits, units, aad_len, 0, 0, out, 1); }
// ---- batch verification (include/zkaes.h): the host back end; zkaes_verify_batch_gpu and the kernel probes are in capi.cpp
int zkaes_verify_batch(const zkaes_vk *vk, const uint8_t *proofs, const size_t *proof_lens, size_t n, const uint8_t *public_input_bits, size_t n_bits, int *accepted_each, size_t *n_accepted) {
    return guard([&] {
        std::unique_ptr<zk::BatchBackend> be = zk::make_host_batch_backend();
        zk::capi::verify_batch_call(vk, proofs, proof_lens, n, public_input_bits, n_bits, accepted_each, n_accepted, *be);
    });
}
int zkaes_verify_batch_timings(double out[8]) {
    return guard([&] {
        if (!out) throw std::invalid_argument("null argument");
        const zk::BatchTimings &t = g_batch_timings;
        out[0] = t.parse_ms; out[1] = t.decompress_ms; out[2] = t.transcripts_ms; out[3] = t.xhat_ms; out[4] = t.msm_ms; out[5] = t.pairing_ms; out[6] = t.total_ms; out[7] = (double)t.sub_batches;
    });
}
// ---- batch verification across keys (include/zkaes.h): the host back end; the _gpu entries and the kernel probe are in capi.cpp
int zkaes_verify_batch_keys(const zkaes_vk *const *vks, size_t n_keys, const uint32_t *key_of, const uint8_t *proofs, const size_t *proof_lens, size_t n, const uint8_t *public_input_bits,
                            const size_t *n_bits_each, int *accepted_each, size_t *n_accepted) {
    return guard([&] {
        std::unique_ptr<zk::BatchBackend> be = zk::make_host_batch_backend();
        zk::capi::verify_batch_keys_call(vks, n_keys, key_of, proofs, proof_lens, n, public_input_bits, n_bits_each, accepted_each, n_accepted, *be);
    });
}
int zkaes_gcm_segment_public_inputs(size_t n_segments, size_t c, const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const uint8_t *ct, size_t ct_len, const uint8_t tag[16],
                                    const uint8_t *commitments, size_t commitments_len, const uint8_t *mask, size_t mask_len, const uint8_t *revealed, uint8_t *out_bits, size_t *n_bits_each,
                                    int *roles) {
    return guard([&] {
        const SegShape S = gcm_segments_shape("gcm_segment_public_inputs", false, nullptr, nullptr, nullptr, n_segments, c, iv, aad, aad_len, ct, ct_len, tag, commitments, commitments_len,
                                              mask != nullptr, mask, mask_len, revealed, ct_len);
        std::vector<uint8_t> bits;
        std::vector<size_t> lens;
        std::vector<int> rl;
        gcm_segment_rows(S, c, iv, aad, aad_len, ct, tag, commitments, mask, revealed, out_bits ? &bits : nullptr, lens, rl);
        for (size_t s = 0; s < S.n; s++) { if (n_bits_each) n_bits_each[s] = lens[s]; if (roles) roles[s] = rl[s]; }
        if (out_bits && !bits.empty()) memcpy(out_bits, bits.data(), bits.size());
    });
}
int zkaes_verify_gcm_segments_batch(const zkaes_vk *head, const zkaes_vk *mid_or_null, const zkaes_vk *tail, const uint8_t *proofs, const size_t *proof_lens, size_t n_segments, size_t c,
                                    const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const uint8_t *ct, size_t ct_len, const uint8_t tag[16], const uint8_t *commitments,
                                    size_t commitments_len, const uint8_t *mask, size_t mask_len, const uint8_t *revealed, size_t revealed_len, int *accepted_each, size_t *n_accepted) {
    return guard([&] {
        std::unique_ptr<zk::BatchBackend> be = zk::make_host_batch_backend();
        zk::capi::verify_gcm_segments_batch_call("verify_gcm_segments_batch", head, mid_or_null, tail, proofs, proof_lens, n_segments, c, iv, aad, aad_len, ct, ct_len, tag, commitments,
                                                 commitments_len, mask, mask_len, revealed, revealed_len, accepted_each, n_accepted, *be);
    });
}
// the rows of a chunked job for batch verification; with a mask (the _rv form) every row ends in the chunk's slice of the mask and of the revealed bytes
static int chunk_public_inputs(const char *entry, int circuit_kind, size_t n_chunks, const uint8_t *iv_or_icb, const uint8_t *ct, size_t ct_len, const uint8_t *key_tag, size_t key_tag_len,
                               const uint8_t *states, const uint8_t *mask, const uint8_t *revealed, uint8_t *out_bits, size_t *n_bits) {
    return guard([&] {
        if (!ct) throw std::invalid_argument("null argument");
        const size_t chunk = require_slices(entry, nullptr, circuit_kind, iv_or_icb, n_chunks, ct_len, key_tag, key_tag_len, false);
        if (mask) zk::require_revealed(mask, revealed, ct_len);
        const size_t row = (iv_or_icb ? 128 : 0) + 8 * chunk + 8 * key_tag_len + (states ? 512 : 0) + (mask ? 8 * zk::mask_bytes(chunk) + 8 * chunk : 0);
        if (n_bits) *n_bits = row;
        if (!out_bits) return;
        for (size_t j = 0; j < n_chunks; j++) {
            std::vector<zk::Fr> pub = chunk_public_input(circuit_kind, j, chunk, iv_or_icb, ct, key_tag, key_tag_len, states, mask, revealed);
            for (size_t i = 0; i < row; i++) out_bits[j * row + i] = pub[i].is_zero() ? 0 : 1;
        }
    });
}
int zkaes_chunk_public_inputs(int circuit_kind, size_t n_chunks, const uint8_t *iv_or_icb, const uint8_t *ct, size_t ct_len, const uint8_t *key_tag, size_t key_tag_len, const uint8_t *states,
                              uint8_t *out_bits, size_t *n_bits) {
    return chunk_public_inputs("chunk_public_inputs", circuit_kind, n_chunks, iv_or_icb, ct, ct_len, key_tag, key_tag_len, states, nullptr, nullptr, out_bits, n_bits);
}
int zkaes_chunk_public_inputs_rv(int circuit_kind, size_t n_chunks, const uint8_t *iv_or_icb, const uint8_t *ct, size_t ct_len, const uint8_t *key_tag, size_t key_tag_len, const uint8_t *states,
                                 const uint8_t *mask, size_t mask_len, const uint8_t *revealed, uint8_t *out_bits, size_t *n_bits) {
    if (!mask || !revealed || mask_len != zk::mask_bytes(ct_len)) return guard([&] { throw std::invalid_argument("chunk_public_inputs_rv: ONE mask over the whole job (ceil(ct_len / 8) bytes) and its revealed bytes"); });
    return chunk_public_inputs("chunk_public_inputs_rv", circuit_kind, n_chunks, iv_or_icb, ct, ct_len, key_tag, key_tag_len, states, mask, revealed, out_bits, n_bits);
}
static int circuit_matrix_gcm_seg(int role, unsigned key_bits, size_t units, size_t aad_len, unsigned reveal, unsigned key_tag_blocks, int which, uint64_t *n_rows, uint64_t *nnz, uint32_t *rowptr,
                                  uint32_t *col, int64_t *coeff, int digest = 0) {
    return guard([&] {
        zk::Circuit c = zk::compile_aes_gcm_segment_circuit(role, units, aad_len, key_bits, reveal > 1 ? 2 : (int)reveal, key_tag_blocks, digest);
        const zk::CsrMatrix &m = which == 0 ? c.A : which == 1 ? c.B : c.C;
        if (n_rows) *n_rows = m.rows();
        if (nnz) *nnz = m.nnz();
        if (rowptr) memcpy(rowptr, m.rowptr.data(), m.rowptr.size() * 4);
        if (col) memcpy(col, m.col.data(), m.col.size() * 4);
        if (coeff) memcpy(coeff, m.coeff.data(), m.coeff.size() * 8);
    });
}
int zkaes_circuit_matrix_gcm_seg(int role, unsigned key_bits, size_t units, size_t aad_len, int which, uint64_t *n_rows, uint64_t *nnz, uint32_t *rowptr, uint32_t *col, int64_t *coeff) {
    return circuit_matrix_gcm_seg(role, key_bits, units, aad_len, 0, 0, which, n_rows, nnz, rowptr, col, coeff);
}
int zkaes_circuit_matrix_gcm_seg_rv(int role, unsigned key_bits, unsigned reveal, size_t units, size_t aad_len, int which, uint64_t *n_rows, uint64_t *nnz, uint32_t *rowptr, uint32_t *col,
                                    int64_t *coeff) {
    return circuit_matrix_gcm_seg(role, key_bits, units, aad_len, reveal, 0, which, n_rows, nnz, rowptr, col, coeff);
}
int zkaes_circuit_matrix_gcm_seg_kt(int role, unsigned key_bits, unsigned reveal, unsigned key_tag_blocks, size_t units, size_t aad_len, int which, uint64_t *n_rows, uint64_t *nnz, uint32_t *rowptr,
                                    uint32_t *col, int64_t *coeff) {
    return circuit_matrix_gcm_seg(role, key_bits, units, aad_len, reveal, key_tag_blocks, which, n_rows, nnz, rowptr, col, coeff);
}
int zkaes_circuit_matrix_gcm_seg_dg(int role, unsigned key_bits, size_t units, size_t aad_len, int which, uint64_t *n_rows, uint64_t *nnz, uint32_t *rowptr, uint32_t *col, int64_t *coeff) {
    return circuit_matrix_gcm_seg(role, key_bits, units, aad_len, 0, 0, which, n_rows, nnz, rowptr, col, coeff, 1);
}
// ---- digests on segmented records (include/zkaes.h): the record helper, the rows and the verifier of a digest record's nd + 1 proofs
int zkaes_gcm_digest_plan(const uint8_t *msg, size_t len, const uint8_t *key, size_t key_len, const uint8_t iv[12], const uint8_t *aad, size_t aad_len, size_t c, const uint8_t *h_in_or_null,
                          uint64_t digest_prefix, uint8_t *ys, size_t ys_cap, uint8_t *states, size_t states_cap, size_t *n_data_segments) {
    return guard([&] {
        if (!msg || !key || !iv || (aad_len && !aad)) throw std::invalid_argument("null argument");
        require_key_len(key_len);
        if (len == 0 || len > ((size_t)1 << 20)) throw std::invalid_argument("GCM segments: a record has 1 .. 2^20 bytes");
        if (c == 0 || c % 4) throw std::invalid_argument("GCM digest segments: a digest segment holds whole 64-byte blocks: c must be a multiple of 4");
        if (len <= 16 * c) throw std::invalid_argument("GCM digest segments: this record fits one segment; a record that fits one proof takes a lone GCM key with a final digest (zkaes_synthesize_keys_pd)");
        if (digest_prefix % 64 || digest_prefix >= ((uint64_t)1 << 61) - len) throw std::invalid_argument("zkaes_gcm_digest_plan: digest_prefix must be a multiple of 64 with digest_prefix + the record's length below 2^61");
        const size_t nd = (len + 16 * c - 1) / (16 * c);
        if (n_data_segments) *n_data_segments = nd;
        if (!ys && !states) return;
        if (!ys || !states || ys_cap < 16 * nd || states_cap < 32 * (nd + 1)) throw std::invalid_argument("gcm_digest_plan: ys takes 16 bytes per data segment and states 32 bytes per data segment and 32 more");
        zk::gcm_digest_plan_host(msg, len, key, key_len, iv, aad, aad_len, c, h_in_or_null, digest_prefix, ys, states);
    });
}
int zkaes_gcm_segment_digest_public_inputs(size_t n_proofs, size_t c, const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const uint8_t *ct, size_t ct_len, const uint8_t tag[16],
                                           const uint8_t *commitments, size_t commitments_len, const uint8_t *states, size_t states_len, uint64_t digest_prefix, uint8_t *out_bits,
                                           size_t *n_bits_each, int *roles) {
    return guard([&] {
        const DgShape S = gcm_digest_shape("gcm_segment_digest_public_inputs", false, nullptr, nullptr, nullptr, nullptr, n_proofs, c, iv, aad, aad_len, ct, ct_len, tag, commitments, commitments_len,
                                           states, states_len, digest_prefix);
        for (size_t s = 0; s <= S.nd; s++) {
            const std::vector<zk::Fr> pub = gcm_digest_public_input(s, S, c, iv, aad, aad_len, ct, tag, commitments, states);
            if (n_bits_each) n_bits_each[s] = pub.size();
            if (roles) roles[s] = s == 0 ? 0 : s < S.nd - 1 ? 1 : s == S.nd - 1 ? 3 : 2;
            if (out_bits) for (const zk::Fr &v : pub) *out_bits++ = v.is_zero() ? 0 : 1;
        }
    });
}
// Proof s < nd is checked against (iv, ctr0 = 2 + s c, its slice of the ciphertext), the aad (head), commitments[s - 1] (mid, last) and commitments[s], then
// (states[s], states[s + 1]) and, for the last, total_bits = 8 (digest_prefix + ct_len) as the verifier computes it HERE; proof nd, the closing tail, against (iv,
// ctr0 = 2 + nd c), the length block built from the lengths seen here, the tag and commitments[nd - 1].  ONE commitments array (nd) and ONE states array (nd + 1) serve
// both sides of every boundary.  A proof that does not parse is a rejected segment
int zkaes_verify_gcm_segments_digest(const zkaes_vk *head, const zkaes_vk *mid_or_null, const zkaes_vk *last, const zkaes_vk *tail, const uint8_t *proofs, const size_t *proof_lens, size_t n_proofs,
                                     size_t c, const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const uint8_t *ct, size_t ct_len, const uint8_t tag[16], const uint8_t *commitments,
                                     size_t commitments_len, const uint8_t *states, size_t states_len, uint64_t digest_prefix, int *accepted_each, size_t *n_accepted) {
    return guard([&] {
        if (n_accepted) *n_accepted = 0;
        if (accepted_each) for (size_t s = 0; s < n_proofs; s++) accepted_each[s] = 0;
        if (!proofs || !proof_lens) throw std::invalid_argument("null argument");
        const DgShape S = gcm_digest_shape("verify_gcm_segments_digest", true, head, mid_or_null, last, tail, n_proofs, c, iv, aad, aad_len, ct, ct_len, tag, commitments, commitments_len, states,
                                           states_len, digest_prefix);
        verify_each(proofs, proof_lens, S.nd + 1, accepted_each, n_accepted, [&](size_t s, const zk::Proof &p) {
            return zk::verify(s == 0 ? head->vk : s < S.nd - 1 ? mid_or_null->vk : s == S.nd - 1 ? last->vk : tail->vk, gcm_digest_public_input(s, S, c, iv, aad, aad_len, ct, tag, commitments, states), p);
        });
    });
}
// ---- key tags on segmented records (include/zkaes.h): the rows and the verifiers of a record whose head carries a key tag.  mask = NULL: plain keys
int zkaes_gcm_segment_public_inputs_kt(size_t n_segments, size_t c, const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const uint8_t *ct, size_t ct_len, const uint8_t tag[16],
                                       const uint8_t *commitments, size_t commitments_len, const uint8_t *key_tag, size_t key_tag_len, const uint8_t *mask, size_t mask_len,
                                       const uint8_t *revealed, uint8_t *out_bits, size_t *n_bits_each, int *roles) {
    return guard([&] {
        if (!key_tag) throw std::invalid_argument("null argument");
        const SegShape S = gcm_segments_shape("gcm_segment_public_inputs_kt", false, nullptr, nullptr, nullptr, n_segments, c, iv, aad, aad_len, ct, ct_len, tag, commitments, commitments_len,
                                              mask != nullptr, mask, mask_len, revealed, ct_len, key_tag, key_tag_len);
        std::vector<uint8_t> bits;
        std::vector<size_t> lens;
        std::vector<int> rl;
        gcm_segment_rows(S, c, iv, aad, aad_len, ct, tag, commitments, mask, revealed, out_bits ? &bits : nullptr, lens, rl, key_tag, key_tag_len);
        for (size_t s = 0; s < S.n; s++) { if (n_bits_each) n_bits_each[s] = lens[s]; if (roles) roles[s] = rl[s]; }
        if (out_bits && !bits.empty()) memcpy(out_bits, bits.data(), bits.size());
    });
}
int zkaes_verify_gcm_segments_kt(const zkaes_vk *head, const zkaes_vk *mid_or_null, const zkaes_vk *tail, const uint8_t *proofs, const size_t *proof_lens, size_t n_segments, size_t c,
                                 const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const uint8_t *ct, size_t ct_len, const uint8_t tag[16], const uint8_t *commitments,
                                 size_t commitments_len, const uint8_t *key_tag, size_t key_tag_len, const uint8_t *mask, size_t mask_len, const uint8_t *revealed, size_t revealed_len,
                                 int *accepted_each, size_t *n_accepted) {
    return guard([&] {
        if (n_accepted) *n_accepted = 0;
        if (accepted_each) for (size_t s = 0; s < n_segments; s++) accepted_each[s] = 0;
        if (!key_tag) throw std::invalid_argument("null argument");
        verify_gcm_segments("verify_gcm_segments_kt", head, mid_or_null, tail, proofs, proof_lens, n_segments, c, iv, aad, aad_len, ct, ct_len, tag, commitments, commitments_len, mask != nullptr,
                            mask, mask_len, revealed, revealed_len, accepted_each, n_accepted, key_tag, key_tag_len);
    });
}
int zkaes_verify_gcm_segments_batch_kt(const zkaes_vk *head, const zkaes_vk *mid_or_null, const zkaes_vk *tail, const uint8_t *proofs, const size_t *proof_lens, size_t n_segments, size_t c,
                                       const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const uint8_t *ct, size_t ct_len, const uint8_t tag[16], const uint8_t *commitments,
                                       size_t commitments_len, const uint8_t *key_tag, size_t key_tag_len, const uint8_t *mask, size_t mask_len, const uint8_t *revealed, size_t revealed_len,
                                       int *accepted_each, size_t *n_accepted) {
    return guard([&] {
        if (n_accepted) *n_accepted = 0;
        if (accepted_each) for (size_t s = 0; s < n_segments; s++) accepted_each[s] = 0;
        if (!key_tag) throw std::invalid_argument("null argument");
        std::unique_ptr<zk::BatchBackend> be = zk::make_host_batch_backend();
        zk::capi::verify_gcm_segments_batch_call("verify_gcm_segments_batch_kt", head, mid_or_null, tail, proofs, proof_lens, n_segments, c, iv, aad, aad_len, ct, ct_len, tag, commitments,
                                                 commitments_len, mask, mask_len, revealed, revealed_len, accepted_each, n_accepted, *be, key_tag, key_tag_len);
    });
}

}  // extern "C"
