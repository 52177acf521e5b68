// tests/keytag_trace_emu.cpp -- k_key_tag_trace of csrc/kernels_witness.cuh behind each mode's own trace kernel(s), and k_witness_expand, run lane by lane ON THE HOST:
// tests/test_keytag_host.py builds this file, which includes that header behind tests/lane_emu.h, with -fsanitize=address,undefined.
// Shapes: ECB-128 16 B T = 1, ECB-256 16 B T = 2, CBC-192 32 B T = 1, CTR-128 17 B T = 2, GCM-256 (17, 5) T = 1; two proofs with different keys per launch; the message,
// key and header buffers hold exactly the bytes that exist, on the heap, and guard bytes lie behind the traces.
// Checked per shape: the tagged circuit's header (T, the tag offset = the untagged circuit's trace length rounded up to 16, the trace length); every byte of the tag
// slots has exactly one writing lane and no lane of the tag kernel writes anywhere else (each lane is run alone over traces prefilled with two different patterns); lanes
// beyond the grid write nothing.  Per proof: every row of (A z) o (B z) = C z holds; the instance is One, the mode's public bits from the host cipher, then the bits of
// zkaes_key_tag for that proof's key, then zero padding; one flipped tag bit of the instance leaves exactly one row unsatisfied; the slots hold D_t, D_t ^ key and the tag.
// No GPU: what the device adds is the launch.
#include "circuit.hpp"
#include "trace_layout.h"
#include "../include/zkaes.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "lane_emu.h"
#include "kernels_witness.cuh"
using namespace zk;
using namespace zk::gpu;
static long long rowdot(const CsrMatrix &m, size_t r, const std::vector<uint8_t> &z) { long long a = 0; for (uint32_t i = m.rowptr[r]; i < m.rowptr[r + 1]; i++) a += z[m.col[i]] ? m.coeff[i] : 0; return a; }
static size_t unsatisfied(const Circuit &c, const std::vector<uint8_t> &z) {
    size_t bad = 0;
    for (size_t r = 0; r < c.num_constraints; r++) if (rowdot(c.A, r, z) * rowdot(c.B, r, z) != rowdot(c.C, r, z)) bad++;
    return bad;
}
static uint8_t sb[256];
enum Mode { ECB, CBC, CTR, GCM };
static const char *mode_name[4] = {"ecb", "cbc", "ctr", "gcm"};
static const uint8_t D_PREFIX[11] = {0x7a, 0x6b, 0x61, 0x65, 0x73, 0x2d, 0x6b, 0x65, 0x79, 0x74, 0x61};

template <int NK>
static void mode_kernels(Mode mode, uint8_t *trace, size_t stride, const uint8_t *msgs, const uint8_t *keys, const uint8_t *pub, uint32_t nproofs, size_t nb, size_t na, size_t L, size_t A) {
    const uint32_t lanes = nproofs * (uint32_t)(mode == GCM ? nb + 3 : nb + 1), ghash_lanes = nproofs * (uint32_t)(na + nb + 2) * 16;
    for (uint32_t t = 0; t < lanes; t++) {
        blockIdx.x = t;
        if (mode == ECB) k_aes_trace<false, NK>(trace, stride, msgs, keys, nullptr, nproofs, (uint32_t)nb, sb);
        else if (mode == CBC) k_aes_trace<true, NK>(trace, stride, msgs, keys, pub, nproofs, (uint32_t)nb, sb);
        else if (mode == CTR) k_aes_trace_ctr<NK>(trace, stride, msgs, keys, pub, nproofs, (uint32_t)nb, (uint32_t)L, sb);
        else k_aes_trace_gcm<NK>(trace, stride, msgs, keys, pub, nproofs, (uint32_t)nb, (uint32_t)na, (uint32_t)L, (uint32_t)A, sb);
    }
    if (mode == GCM) for (uint32_t t = 0; t < ghash_lanes; t++) { blockIdx.x = t; k_ghash_trace<NK>(trace, stride, nproofs, (uint32_t)nb, (uint32_t)na, (uint32_t)L, (uint32_t)A); }
}

template <int NK>
static void run(Mode mode, size_t L, size_t A, size_t T, int &bad_total) {
    const size_t kb = 4 * NK, nb = (L + 15) / 16, na = (A + 15) / 16, hs = 12 + A;
    auto compile = [&](size_t t) { return mode == ECB ? compile_aes_circuit(L, 8 * kb, t) : mode == CBC ? compile_aes_cbc_circuit(L, 8 * kb, t) : mode == CTR ? compile_aes_ctr_circuit(L, 8 * kb, t) : compile_aes_gcm_circuit(L, A, 8 * kb, t); };
    const Circuit c = compile(T), plain = compile(0);
    const size_t mode_bytes = mode == ECB ? TRK_ECB_BYTES(NK, nb) : mode == CBC ? TRK_CBC_BYTES(NK, nb) : mode == CTR ? TRK_CTR_BYTES(NK, nb) : TRK_GCM_BYTES(NK, na, nb);
    const size_t slot = TRK_BLOCK_STRIDE(NK), tag_off = (mode_bytes + 15) / 16 * 16;
    if (plain.trace_bytes != mode_bytes || plain.key_tag_blocks != 0 || plain.key_tag_off != 0 || c.key_tag_blocks != T || c.key_tag_off != tag_off || c.trace_bytes != tag_off + T * slot ||
        c.trace_bytes % 16 || c.raw_instance != plain.raw_instance + 128 * T || c.sbox_in_off.size() != plain.sbox_in_off.size() + T * TRK_SBOX_PER_BLOCK(NK) || c.message_bytes != L) {
        printf("NK=%d %s L=%zu A=%zu T=%zu: circuit header is off\n", NK, mode_name[mode], L, A, T); bad_total++;
    }
    const uint32_t nproofs = 2;
    const size_t pub_each = mode == GCM ? hs : 16, stride = c.trace_bytes, total = stride * nproofs + 64;
    std::unique_ptr<uint8_t[]> msgs(new uint8_t[L * nproofs]), keys(new uint8_t[kb * nproofs]), pub(new uint8_t[pub_each * nproofs]);      // exactly the bytes that exist
    srand(7000 * NK + 10 * (unsigned)mode + (unsigned)L + (unsigned)T);
    for (size_t i = 0; i < L * nproofs; i++) msgs[i] = (uint8_t)rand();
    for (size_t i = 0; i < kb * nproofs; i++) keys[i] = (uint8_t)rand();                             // two different keys
    for (size_t i = 0; i < pub_each * nproofs; i++) pub[i] = (uint8_t)rand();
    // ---- who writes what: each lane of the tag kernel alone, over two prefill patterns (a byte is written iff it leaves either pattern)
    const uint32_t tag_lanes = nproofs * (uint32_t)T;
    std::vector<uint32_t> writers(total, 0);
    for (uint32_t t = 0; t < tag_lanes + 3; t++) {
        std::vector<uint8_t> a(total, 0xAA), b(total, 0x55);
        blockIdx.x = t;
        k_key_tag_trace<NK>(a.data(), stride, tag_off, keys.get(), nproofs, (uint32_t)T, sb);
        k_key_tag_trace<NK>(b.data(), stride, tag_off, keys.get(), nproofs, (uint32_t)T, sb);
        size_t wrote = 0;
        for (size_t i = 0; i < total; i++) if (a[i] != 0xAA || b[i] != 0x55) { writers[i]++; wrote++; }
        if (t >= tag_lanes && wrote) { printf("a tag lane beyond the grid wrote to the trace\n"); bad_total++; }
        if (t < tag_lanes && wrote != slot) { printf("tag lane %u wrote %zu bytes, a slot has %zu\n", t, wrote, slot); bad_total++; }
    }
    size_t wrong_writers = 0;
    for (size_t i = 0; i < total; i++) {
        const size_t p = i / stride, in = i % stride;
        const bool tag_byte = p < nproofs && in >= tag_off;                                        // (tag_off + T slots = stride)
        wrong_writers += writers[i] != (tag_byte ? 1u : 0u);
    }
    printf("NK=%d %s L=%zu A=%zu T=%zu: bytes whose writer count is off %zu\n", NK, mode_name[mode], L, A, T, wrong_writers);
    bad_total += wrong_writers != 0;
    // ---- the launch as the library makes it: the mode's kernel(s), then the tag kernel; the bytes ahead of the tag slots stay what the mode's kernels left
    std::vector<uint8_t> trace(total, 0xAA);
    mode_kernels<NK>(mode, trace.data(), stride, msgs.get(), keys.get(), pub.get(), nproofs, nb, na, L, A);
    const std::vector<uint8_t> before(trace);
    for (uint32_t t = 0; t < tag_lanes + 3; t++) { blockIdx.x = t; k_key_tag_trace<NK>(trace.data(), stride, tag_off, keys.get(), nproofs, (uint32_t)T, sb); }
    size_t touched_outside = 0, untouched_inside = 0;
    for (size_t i = 0; i < total; i++) {
        const bool tag_byte = i / stride < nproofs && i % stride >= tag_off;
        if (!tag_byte) touched_outside += trace[i] != before[i];
        else untouched_inside += before[i] != 0xAA;                                                // the mode's kernels stay out of the slots
    }
    // the same mode kernels at the untagged key's stride give the same bytes ahead of the slots
    std::vector<uint8_t> plain_trace(plain.trace_bytes * nproofs + 64, 0xAA);
    mode_kernels<NK>(mode, plain_trace.data(), plain.trace_bytes, msgs.get(), keys.get(), pub.get(), nproofs, nb, na, L, A);
    size_t differs_from_plain = 0;
    for (uint32_t p = 0; p < nproofs; p++) differs_from_plain += memcmp(trace.data() + p * stride, plain_trace.data() + p * plain.trace_bytes, plain.trace_bytes) != 0;
    printf("NK=%d %s L=%zu A=%zu T=%zu: bytes outside the slots touched %zu, slot bytes the mode's kernels wrote %zu, proofs whose head differs from the untagged trace %zu\n", NK, mode_name[mode], L, A,
           T, touched_outside, untouched_inside, differs_from_plain);
    bad_total += (touched_outside != 0) + (untouched_inside != 0) + (differs_from_plain != 0);
    for (uint32_t p = 0; p < nproofs; p++) {
        const uint8_t *tr = trace.data() + p * stride, *key = keys.get() + kb * p, *msg = msgs.get() + L * p, *pb = pub.get() + pub_each * p;
        std::vector<uint8_t> z(c.num_variables());
        for (uint32_t i = 0; i < z.size(); i++) { blockIdx.x = i; k_witness_expand(z.data(), c.desc.data(), (uint32_t)z.size(), tr, c.sbox_in_off.data(), c.sbox_tmpl.data(), sb); }
        size_t bad = unsatisfied(c, z);
        std::vector<uint8_t> ct(L), want_pub;
        uint8_t gtag[16], ktag[32];
        if (mode == ECB) aes_ecb_encrypt_host(msg, L, key, kb, ct.data());
        else if (mode == CBC) aes128_cbc_encrypt_host(msg, L, key, pb, ct.data(), kb);
        else if (mode == CTR) aes128_ctr_crypt_host(msg, L, key, pb, ct.data(), kb);
        else aes128_gcm_encrypt_host(msg, L, key, pb, A ? pb + 12 : nullptr, A, ct.data(), gtag, kb);
        if (zkaes_key_tag(key, kb, T, ktag) != 0) { printf("zkaes_key_tag failed: %s\n", zkaes_last_error()); bad_total++; }
        if (mode != ECB) want_pub.assign(pb, pb + pub_each);
        want_pub.insert(want_pub.end(), ct.begin(), ct.end());
        if (mode == GCM) want_pub.insert(want_pub.end(), gtag, gtag + 16);
        const size_t tag_at = 1 + 8 * want_pub.size();
        want_pub.insert(want_pub.end(), ktag, ktag + 16 * T);
        size_t ibad = z[0] != 1, at = 1;
        for (uint8_t b : want_pub) for (int k = 0; k < 8; k++) ibad += z[at++] != ((b >> k) & 1);
        if (at != c.raw_instance || tag_at + 128 * T != c.raw_instance) ibad++;
        for (; at < c.num_instance; at++) ibad += z[at] != 0;
        // the slots: D_t, D_t ^ key, the tag
        for (size_t t = 0; t < T; t++) {
            const uint8_t *bl = tr + tag_off + t * slot;
            uint8_t d[16] = {0};
            memcpy(d, D_PREFIX, 11); d[11] = (uint8_t)t;
            ibad += memcmp(bl + TR_BL_MSG, d, 16) != 0;
            for (int i = 0; i < 16; i++) ibad += bl[TR_BL_S + i] != (uint8_t)(d[i] ^ key[i]);
            ibad += memcmp(bl + TRK_BL_CT(NK), ktag + 16 * t, 16) != 0;
        }
        std::vector<uint8_t> zf(z);
        zf[tag_at + 128 * (T - 1) + 8 * 15 + 3] ^= 1;                                               // a bit of the last tag byte
        size_t flip_tag = unsatisfied(c, zf);
        printf("NK=%d %s L=%zu A=%zu T=%zu proof %u: unsatisfied %zu, instance mismatches %zu, rows unsatisfied after a tag flip %zu\n", NK, mode_name[mode], L, A, T, p, bad, ibad, flip_tag);
        bad_total += (int)(bad + ibad) + (flip_tag != 1);
    }
}

int main() {
    for (int i = 0; i < 256; i++) sb[i] = aes_sbox_value((uint8_t)i);
    int bad_total = 0;
    run<4>(ECB, 16, 0, 1, bad_total);
    run<8>(ECB, 16, 0, 2, bad_total);
    run<6>(CBC, 32, 0, 1, bad_total);
    run<4>(CTR, 17, 0, 2, bad_total);
    run<8>(GCM, 17, 5, 1, bad_total);
    printf("total bad %d\n", bad_total);
    return bad_total != 0;
}
