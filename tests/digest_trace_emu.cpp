// tests/digest_trace_emu.cpp -- k_sha256_trace of csrc/kernels_digest.cuh behind each mode's own trace kernel(s) and the key-tag kernel, and k_witness_expand, run lane by
// lane ON THE HOST: tests/test_digest_host.py builds this file, which includes the two kernel headers behind tests/lane_emu.h, with
// -fsanitize=address,undefined.  Shapes (mode, key bits, L, A, T, digest kind, P): ECB-128 64 T = 0 chain; ECB-128 128 T = 0 chain (the second lane re-walks, the midstate
// is a witness); CTR-128 17 T = 1 final; CTR-128 55 and 56 T = 0 final (one compression / two); CBC-192 64 T = 1 chain; GCM-256 (17, 5) T = 1 final P = 64; ECB-256 64
// T = 2 chain.  Two proofs with different keys, messages, headers and H_in per launch (proof 0 starts from SHA-256's initial value except for CBC); the message, key and
// header buffers hold exactly the bytes that exist, on the heap, and guard bytes lie behind the traces.
// Checked per shape: the circuit's header (kind, prefix, compressions, the region's offset = the undigested circuit's trace length rounded up to 16, the trace length,
// 512 more instance bits); every byte of the digest region has exactly one writing lane and no lane of the digest kernel writes anywhere else (each lane is run alone
// over traces prefilled with two different patterns); lanes beyond the grid write nothing; the bytes ahead of the region are what the undigested key's kernels leave.
// Per proof: every row of (A z) o (B z) = C z holds; the instance is One, the undigested circuit's public bits, H_in, then H_out from the host's SHA-256, then zero
// padding; one flipped H_out bit of the instance leaves exactly one row unsatisfied, one flipped H_in bit at least one.  No GPU: what the device adds is the launch.
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
#include "kernels_digest.cuh"
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

// the launch as the library makes it ahead of the digest kernel: the mode's kernel(s), then the tag kernel
template <int NK>
static void mode_kernels(Mode mode, uint8_t *trace, size_t stride, const uint8_t *msgs, const uint8_t *keys, const uint8_t *pub, uint32_t nproofs, size_t nb, size_t na, size_t L, size_t A, size_t T, size_t tag_off) {
    const uint32_t lanes = nproofs * (uint32_t)(mode == GCM ? nb + 3 : nb + 1), ghash_lanes = nproofs * (uint32_t)(na + nb + 2) * 16;
    for (uint32_t t = 0; t < lanes; t++) {
        blockIdx.x = t;
        if (mode == ECB) k_aes_trace<false, NK>(trace, stride, msgs, keys, nullptr, nproofs, (uint32_t)nb, sb);
        else if (mode == CBC) k_aes_trace<true, NK>(trace, stride, msgs, keys, pub, nproofs, (uint32_t)nb, sb);
        else if (mode == CTR) k_aes_trace_ctr<NK>(trace, stride, msgs, keys, pub, nproofs, (uint32_t)nb, (uint32_t)L, sb);
        else k_aes_trace_gcm<NK>(trace, stride, msgs, keys, pub, nproofs, (uint32_t)nb, (uint32_t)na, (uint32_t)L, (uint32_t)A, sb);
    }
    if (mode == GCM) for (uint32_t t = 0; t < ghash_lanes; t++) { blockIdx.x = t; k_ghash_trace<NK>(trace, stride, nproofs, (uint32_t)nb, (uint32_t)na, (uint32_t)L, (uint32_t)A); }
    for (uint32_t t = 0; t < nproofs * (uint32_t)T; t++) { blockIdx.x = t; k_key_tag_trace<NK>(trace, stride, tag_off, keys, nproofs, (uint32_t)T, sb); }
}

template <int NK>
static void run(Mode mode, size_t L, size_t A, size_t T, int kind, uint64_t P, int &bad_total) {
    const size_t kb = 4 * NK, nb = (L + 15) / 16, na = (A + 15) / 16;
    auto compile = [&](int d, uint64_t p) {
        return mode == ECB ? compile_aes_circuit(L, 8 * kb, T, d, p) : mode == CBC ? compile_aes_cbc_circuit(L, 8 * kb, T, d, p) : mode == CTR ? compile_aes_ctr_circuit(L, 8 * kb, T, d, p)
                                                                                                                                                  : compile_aes_gcm_circuit(L, A, 8 * kb, T, d, p);
    };
    const Circuit c = compile(kind, P), plain = compile(0, 0);
    const size_t nblk = kind == 1 ? L / 64 : (L + 9 + 63) / 64, dg = (plain.trace_bytes + 15) / 16 * 16, region = 64 + nblk * 4032, hb = mode_header_bytes(c);
    char name[96];
    snprintf(name, sizeof name, "NK=%d %s L=%zu A=%zu T=%zu D=%d P=%llu", NK, mode_name[mode], L, A, T, kind, (unsigned long long)P);
    if (c.digest_kind != kind || c.digest_prefix != P || c.digest_blocks != nblk || c.digest_off != dg || c.trace_bytes != dg + region || c.trace_bytes % 16 || plain.digest_kind != 0 || plain.digest_off != 0 ||
        c.raw_instance != plain.raw_instance + 512 || c.key_tag_off != plain.key_tag_off || c.sbox_in_off.size() != plain.sbox_in_off.size() || c.message_bytes != L || hb != (mode == ECB ? 0 : mode == GCM ? 12 + A : 16)) {
        printf("%s: circuit header is off\n", name); bad_total++;
    }
    const uint32_t nproofs = 2;
    const size_t pub_each = hb ? hb : 1, stride = c.trace_bytes, total = stride * nproofs + 64;
    std::unique_ptr<uint8_t[]> msgs(new uint8_t[L * nproofs]), keys(new uint8_t[kb * nproofs]), pub(new uint8_t[pub_each * nproofs]), hdrs(new uint8_t[(hb + 32) * nproofs]);      // exactly the bytes that exist
    srand(9000 * NK + 10 * (unsigned)mode + (unsigned)L + (unsigned)T + 7 * (unsigned)kind);
    for (size_t i = 0; i < L * nproofs; i++) msgs[i] = (uint8_t)rand();
    for (size_t i = 0; i < kb * nproofs; i++) keys[i] = (uint8_t)rand();
    for (size_t i = 0; i < pub_each * nproofs; i++) pub[i] = (uint8_t)rand();
    for (uint32_t p = 0; p < nproofs; p++) {
        uint8_t *h = hdrs.get() + (hb + 32) * p;
        if (hb) memcpy(h, pub.get() + hb * p, hb);
        if (p == 0 && mode != CBC) sha256_chain(nullptr, nullptr, 0, h + hb);                       // SHA-256's initial value
        else for (int i = 0; i < 32; i++) h[hb + i] = (uint8_t)rand();
    }
    const uint64_t total_bits = 8 * (P + L);
    auto digest_lane = [&](uint8_t *trace, uint32_t t) {
        blockIdx.x = t;
        k_sha256_trace(trace, stride, dg, msgs.get(), hdrs.get(), hb + 32, hb, nproofs, (uint32_t)nblk, (uint32_t)L, (uint32_t)kind, total_bits);
    };
    // ---- who writes what: each lane of the digest kernel alone, over two prefill patterns (a byte is written iff it leaves either pattern)
    const uint32_t lanes = nproofs * (uint32_t)nblk;
    std::vector<uint32_t> writers(total, 0);
    for (uint32_t t = 0; t < lanes + 3; t++) {
        std::vector<uint8_t> a(total, 0xAA), b(total, 0x55);
        digest_lane(a.data(), t);
        digest_lane(b.data(), t);
        size_t wrote = 0;
        for (size_t i = 0; i < total; i++) if (a[i] != 0xAA || b[i] != 0x55) { writers[i]++; wrote++; }
        if (t >= lanes && wrote) { printf("%s: a digest lane beyond the grid wrote to the trace\n", name); bad_total++; }
        const size_t want = 4032 + (t % nblk == 0 ? 32 : 0) + (t % nblk == nblk - 1 ? 32 : 0);
        if (t < lanes && wrote != want) { printf("%s: digest lane %u wrote %zu bytes, not %zu\n", name, t, wrote, want); bad_total++; }
    }
    size_t wrong_writers = 0;
    for (size_t i = 0; i < total; i++) {
        const bool region_byte = i / stride < nproofs && i % stride >= dg;                           // (dg + region = stride)
        wrong_writers += writers[i] != (region_byte ? 1u : 0u);
    }
    // ---- the launch as the library makes it; the bytes ahead of the region stay what the undigested key's kernels leave
    std::vector<uint8_t> trace(total, 0xAA);
    mode_kernels<NK>(mode, trace.data(), stride, msgs.get(), keys.get(), pub.get(), nproofs, nb, na, L, A, T, c.key_tag_off);
    const std::vector<uint8_t> before(trace);
    for (uint32_t t = 0; t < lanes + 3; t++) digest_lane(trace.data(), t);
    size_t touched_outside = 0, untouched_inside = 0, differs_from_plain = 0;
    for (size_t i = 0; i < total; i++) {
        const bool region_byte = i / stride < nproofs && i % stride >= dg;
        if (!region_byte) touched_outside += trace[i] != before[i];
        else untouched_inside += before[i] != 0xAA;                                                 // the other kernels stay out of the region
    }
    std::vector<uint8_t> plain_trace(plain.trace_bytes * nproofs + 64, 0xAA);
    mode_kernels<NK>(mode, plain_trace.data(), plain.trace_bytes, msgs.get(), keys.get(), pub.get(), nproofs, nb, na, L, A, T, plain.key_tag_off);
    for (uint32_t p = 0; p < nproofs; p++) differs_from_plain += memcmp(trace.data() + p * stride, plain_trace.data() + p * plain.trace_bytes, plain.trace_bytes) != 0;
    printf("%s: bytes whose writer count is off %zu, bytes outside the region touched %zu, region bytes other kernels wrote %zu, proofs whose head differs from the undigested trace %zu\n", name,
           wrong_writers, touched_outside, untouched_inside, differs_from_plain);
    bad_total += (wrong_writers != 0) + (touched_outside != 0) + (untouched_inside != 0) + (differs_from_plain != 0);
    for (uint32_t p = 0; p < nproofs; p++) {
        const uint8_t *tr = trace.data() + p * stride, *msg = msgs.get() + L * p, *hin = hdrs.get() + (hb + 32) * p + hb;
        std::vector<uint8_t> z(c.num_variables()), zp(plain.num_variables());
        for (uint32_t i = 0; i < z.size(); i++) { blockIdx.x = i; k_witness_expand(z.data(), c.desc.data(), (uint32_t)z.size(), tr, c.sbox_in_off.data(), c.sbox_tmpl.data(), sb); }
        for (uint32_t i = 0; i < zp.size(); i++) { blockIdx.x = i; k_witness_expand(zp.data(), plain.desc.data(), (uint32_t)zp.size(), plain_trace.data() + p * plain.trace_bytes, plain.sbox_in_off.data(), plain.sbox_tmpl.data(), sb); }
        const size_t bad = unsatisfied(c, z);
        uint8_t hout[32];
        if (kind == 1) sha256_chain(hin, msg, L, hout); else sha256_finish(hin, P, msg, L, hout);
        // the instance: the undigested circuit's, then H_in, H_out, then zero padding
        size_t ibad = 0, at = plain.raw_instance;
        for (size_t i = 0; i < plain.raw_instance; i++) ibad += z[i] != zp[i];
        for (int j = 0; j < 32; j++) for (int k = 0; k < 8; k++) ibad += z[at++] != ((hin[j] >> k) & 1);
        const size_t hout_at = at;
        for (int j = 0; j < 32; j++) for (int k = 0; k < 8; k++) ibad += z[at++] != ((hout[j] >> k) & 1);
        if (at != c.raw_instance) ibad++;
        for (; at < c.num_instance; at++) ibad += z[at] != 0;
        ibad += memcmp(tr + dg, hin, 32) != 0;
        ibad += memcmp(tr + dg + 32, hout, 32) != 0;
        std::vector<uint8_t> zf(z);
        zf[hout_at + 8 * (5 + 13 * p) + 3] ^= 1;
        const size_t flip_out = unsatisfied(c, zf);
        zf = z;
        zf[plain.raw_instance + 8 * (2 + 17 * p) + 6] ^= 1;
        const size_t flip_in = unsatisfied(c, zf);
        printf("%s proof %u: unsatisfied %zu, instance mismatches %zu, rows unsatisfied after an H_out flip %zu, after an H_in flip %zu\n", name, p, bad, ibad, flip_out, flip_in);
        bad_total += (int)(bad + ibad) + (flip_out != 1) + (flip_in < 1);
    }
}

int main() {
    for (int i = 0; i < 256; i++) sb[i] = aes_sbox_value((uint8_t)i);
    int bad_total = 0;
    run<4>(ECB, 64, 0, 0, 1, 0, bad_total);
    run<4>(ECB, 128, 0, 0, 1, 0, bad_total);
    run<4>(CTR, 17, 0, 1, 2, 0, bad_total);
    run<4>(CTR, 55, 0, 0, 2, 0, bad_total);
    run<4>(CTR, 56, 0, 0, 2, 0, bad_total);
    run<6>(CBC, 64, 0, 1, 1, 0, bad_total);
    run<8>(GCM, 17, 5, 1, 2, 64, bad_total);
    run<8>(ECB, 64, 0, 2, 1, 0, bad_total);
    printf("total bad %d\n", bad_total);
    return bad_total != 0;
}
