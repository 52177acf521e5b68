// tests/reveal_trace_emu.cpp -- k_reveal_trace of csrc/kernels_reveal.cuh behind each mode's own trace kernel(s), the key-tag kernel and k_sha256_trace, and
// k_witness_expand, run lane by lane ON THE HOST: tests/test_reveal_host.py builds this file, which includes the three kernel headers behind tests/lane_emu.h,
// with -fsanitize=address,undefined.  Shapes (mode, key bits, L, A, T, digest kind): ECB-128 16; CTR-128 1 and 17 with T = 1 and a final digest; CBC-192 32;
// GCM-256 (17, 5); ECB-256 64 with T = 2 and a chain digest.  Masks: all zero, all one, only byte 0, only byte L - 1, bytes 15 and 16 (the lane boundary; the ones that
// exist), alternating -- two proofs with different masks, keys, messages and headers per launch, three launches per shape.  The message, key and header buffers hold
// exactly the bytes that exist, on the heap, and guard bytes lie behind the traces.
// Checked per shape: the circuit's header (the flag, the region's offset = the R = 0 circuit's trace length rounded up to 16, the trace length, 8 ceil(L / 8) + 8 L more
// instance bits, 16 ceil(L / 8) + 15 L more rows, no more witnesses).  Per launch: every byte of the reveal region has exactly one writing lane and no lane of the reveal
// kernel writes anywhere else (each lane is run alone over traces prefilled with two different patterns); lanes beyond the grid write nothing; the bytes ahead of the
// region are what the R = 0 key's kernels leave.  Per proof: every row of (A z) o (B z) = C z holds; the instance is the R = 0 circuit's, then the mask, then revealed
// from the host's masking (statement.hpp), then zero padding; the region holds (mask, zeros, revealed, zeros); one flipped revealed bit leaves exactly one row
// unsatisfied; one flipped mask bit at a revealed non-zero byte at least one.  No GPU: what the device adds is the launch.
#include "circuit.hpp"
#include "statement.hpp"
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
#include "kernels_reveal.cuh"
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
static const char *mask_name[6] = {"zero", "ones", "first", "last", "15+16", "alternating"};

static std::vector<uint8_t> make_mask(int which, size_t L) {
    std::vector<uint8_t> m((L + 7) / 8, 0);
    auto set = [&](size_t i) { if (i < L) m[i / 8] |= (uint8_t)(1u << (i % 8)); };
    for (size_t i = 0; i < L; i++) if (which == 1 || (which == 5 && i % 2 == 0)) set(i);
    if (which == 2) set(0);
    if (which == 3) set(L - 1);
    if (which == 4) { set(15); set(16); }
    return m;
}

// the launch as the library makes it ahead of the reveal kernel: the mode's kernel(s), the tag kernel, the digest kernel
template <int NK>
static void kernels_ahead(Mode mode, uint8_t *trace, size_t stride, const uint8_t *msgs, const uint8_t *keys, const uint8_t *pub, const uint8_t *hdrs, size_t hdr_stride, size_t hb, uint32_t nproofs,
                          size_t L, size_t A, size_t T, int kind, const Circuit &c) {
    const size_t nb = (L + 15) / 16, na = (A + 15) / 16;
    const uint32_t lanes = nproofs * (uint32_t)(mode == GCM ? nb + 3 : nb + 1), ghash_lanes = nproofs * (uint32_t)(na + nb + 2) * 16;
    for (uint32_t t = 0; t < lanes; t++) {
        blockIdx.x = t;
        if (mode == ECB) k_aes_trace<false, NK>(trace, stride, msgs, keys, nullptr, nproofs, (uint32_t)nb, sb);
        else if (mode == CBC) k_aes_trace<true, NK>(trace, stride, msgs, keys, pub, nproofs, (uint32_t)nb, sb);
        else if (mode == CTR) k_aes_trace_ctr<NK>(trace, stride, msgs, keys, pub, nproofs, (uint32_t)nb, (uint32_t)L, sb);
        else k_aes_trace_gcm<NK>(trace, stride, msgs, keys, pub, nproofs, (uint32_t)nb, (uint32_t)na, (uint32_t)L, (uint32_t)A, sb);
    }
    if (mode == GCM) for (uint32_t t = 0; t < ghash_lanes; t++) { blockIdx.x = t; k_ghash_trace<NK>(trace, stride, nproofs, (uint32_t)nb, (uint32_t)na, (uint32_t)L, (uint32_t)A); }
    for (uint32_t t = 0; t < nproofs * (uint32_t)T; t++) { blockIdx.x = t; k_key_tag_trace<NK>(trace, stride, c.key_tag_off, keys, nproofs, (uint32_t)T, sb); }
    if (kind) {
        const uint32_t nblk = (uint32_t)c.digest_blocks;
        for (uint32_t t = 0; t < nproofs * nblk; t++) { blockIdx.x = t; k_sha256_trace(trace, stride, c.digest_off, msgs, hdrs, hdr_stride, hb, nproofs, nblk, (uint32_t)L, (uint32_t)kind, 8 * (uint64_t)L); }
    }
}

template <int NK>
static void run(Mode mode, size_t L, size_t A, size_t T, int kind, int &bad_total) {
    const size_t kb = 4 * NK, mb = (L + 7) / 8, nl = (L + 15) / 16;
    auto compile = [&](int rv) {
        return mode == ECB ? compile_aes_circuit(L, 8 * kb, T, kind, 0, rv) : mode == CBC ? compile_aes_cbc_circuit(L, 8 * kb, T, kind, 0, rv) : mode == CTR ? compile_aes_ctr_circuit(L, 8 * kb, T, kind, 0, rv)
                                                                                                                                                            : compile_aes_gcm_circuit(L, A, 8 * kb, T, kind, 0, rv);
    };
    const Circuit c = compile(1), plain = compile(0);
    const size_t rv = (plain.trace_bytes + 15) / 16 * 16, rev_at = (mb + 15) / 16 * 16, region = rev_at + 16 * nl, hb = mode_header_bytes(c), dgb = kind ? 32 : 0, hs = hb + dgb + mb;
    char name[96];
    snprintf(name, sizeof name, "NK=%d %s L=%zu A=%zu T=%zu D=%d", NK, mode_name[mode], L, A, T, kind);
    if (c.reveal != 1 || plain.reveal != 0 || plain.reveal_off != 0 || c.reveal_off != rv || c.trace_bytes != rv + region || c.trace_bytes % 16 || c.raw_instance != plain.raw_instance + 8 * mb + 8 * L ||
        c.raw_constraints != plain.raw_constraints + 16 * mb + 15 * L || c.raw_witness != plain.raw_witness || c.key_tag_off != plain.key_tag_off || c.digest_off != plain.digest_off || c.message_bytes != L ||
        reveal_mask_bytes(c) != mb || reveal_mask_bytes(plain) != 0 || TRV_BYTES(plain.trace_bytes, 1, L) != c.trace_bytes || TRV_BYTES(plain.trace_bytes, 0, L) != plain.trace_bytes) {
        printf("%s: circuit header is off\n", name); bad_total++;
    }
    const uint32_t nproofs = 2;
    const size_t pub_each = hb ? hb : 1, stride = c.trace_bytes, total = stride * nproofs + 64;
    std::unique_ptr<uint8_t[]> msgs(new uint8_t[L * nproofs]), keys(new uint8_t[kb * nproofs]), pub(new uint8_t[pub_each * nproofs]), hdrs(new uint8_t[hs * nproofs]), plain_hdrs(new uint8_t[(hb + dgb + 1) * nproofs]);
    srand(7000 * NK + 10 * (unsigned)mode + (unsigned)L + (unsigned)T + 7 * (unsigned)kind);
    for (size_t i = 0; i < L * nproofs; i++) msgs[i] = (uint8_t)(rand() | 1);                           // no zero byte: a revealed byte always shows
    for (size_t i = 0; i < kb * nproofs; i++) keys[i] = (uint8_t)rand();
    for (size_t i = 0; i < pub_each * nproofs; i++) pub[i] = (uint8_t)rand();
    std::vector<uint8_t> plain_trace(plain.trace_bytes * nproofs + 64, 0xAA);
    for (int launch = 0; launch < 3; launch++) {
        std::vector<uint8_t> masks[2] = {make_mask(2 * launch, L), make_mask(2 * launch + 1, L)};
        for (uint32_t p = 0; p < nproofs; p++) {
            uint8_t *h = hdrs.get() + hs * p, *ph = plain_hdrs.get() + (hb + dgb) * p;
            if (hb) memcpy(h, pub.get() + hb * p, hb);
            if (kind && p == 0) sha256_chain(nullptr, nullptr, 0, h + hb);
            else for (size_t i = 0; i < dgb; i++) h[hb + i] = (uint8_t)(31 * i + 7 * p + 3);
            memcpy(h + hb + dgb, masks[p].data(), mb);
            memcpy(ph, h, hb + dgb);
        }
        auto reveal_lane = [&](uint8_t *trace, uint32_t t) {
            blockIdx.x = t;
            k_reveal_trace(trace, stride, rv, msgs.get(), hdrs.get(), hs, hb + dgb, nproofs, (uint32_t)nl, (uint32_t)L);
        };
        // ---- who writes what: each lane of the reveal kernel alone, over two prefill patterns (a byte is written iff it leaves either pattern)
        const uint32_t lanes = nproofs * (uint32_t)nl;
        std::vector<uint32_t> writers(total, 0);
        for (uint32_t t = 0; t < lanes + 3; t++) {
            std::vector<uint8_t> a(total, 0xAA), b(total, 0x55);
            reveal_lane(a.data(), t);
            reveal_lane(b.data(), t);
            size_t wrote = 0;
            for (size_t i = 0; i < total; i++) if (a[i] != 0xAA || b[i] != 0x55) { writers[i]++; wrote++; }
            if (t >= lanes && wrote) { printf("%s: a reveal lane beyond the grid wrote to the trace\n", name); bad_total++; }
            const size_t want = 18 + (t % nl == nl - 1 ? rev_at - 2 * nl : 0);
            if (t < lanes && wrote != want) { printf("%s: reveal lane %u wrote %zu bytes, not %zu\n", name, t, wrote, want); bad_total++; }
        }
        size_t wrong_writers = 0;
        for (size_t i = 0; i < total; i++) {
            const bool region_byte = i / stride < nproofs && i % stride >= rv;                           // (rv + region = stride)
            wrong_writers += writers[i] != (region_byte ? 1u : 0u);
        }
        // ---- the launch as the library makes it; the bytes ahead of the region stay what the R = 0 key's kernels leave
        std::vector<uint8_t> trace(total, 0xAA);
        kernels_ahead<NK>(mode, trace.data(), stride, msgs.get(), keys.get(), pub.get(), hdrs.get(), hs, hb, nproofs, L, A, T, kind, c);
        const std::vector<uint8_t> before(trace);
        for (uint32_t t = 0; t < lanes + 3; t++) reveal_lane(trace.data(), t);
        size_t touched_outside = 0, untouched_inside = 0, differs_from_plain = 0;
        for (size_t i = 0; i < total; i++) {
            const bool region_byte = i / stride < nproofs && i % stride >= rv;
            if (!region_byte) touched_outside += trace[i] != before[i];
            else untouched_inside += before[i] != 0xAA;                                                 // the other kernels stay out of the region
        }
        std::fill(plain_trace.begin(), plain_trace.end(), (uint8_t)0xAA);
        kernels_ahead<NK>(mode, plain_trace.data(), plain.trace_bytes, msgs.get(), keys.get(), pub.get(), plain_hdrs.get(), hb + dgb, hb, nproofs, L, A, T, kind, plain);
        for (uint32_t p = 0; p < nproofs; p++) differs_from_plain += memcmp(trace.data() + p * stride, plain_trace.data() + p * plain.trace_bytes, plain.trace_bytes) != 0;
        printf("%s masks %s / %s: bytes whose writer count is off %zu, bytes outside the region touched %zu, region bytes other kernels wrote %zu, proofs whose head differs from the R = 0 trace %zu\n", name,
               mask_name[2 * launch], mask_name[2 * launch + 1], wrong_writers, touched_outside, untouched_inside, differs_from_plain);
        bad_total += (wrong_writers != 0) + (touched_outside != 0) + (untouched_inside != 0) + (differs_from_plain != 0);
        for (uint32_t p = 0; p < nproofs; p++) {
            const uint8_t *tr = trace.data() + p * stride, *msg = msgs.get() + L * p, *mask = masks[p].data();
            std::vector<uint8_t> z(c.num_variables()), zp(plain.num_variables()), revealed(L), want_region(region, 0);
            for (uint32_t i = 0; i < z.size(); i++) { blockIdx.x = i; k_witness_expand(z.data(), c.desc.data(), (uint32_t)z.size(), tr, c.sbox_in_off.data(), c.sbox_tmpl.data(), sb); }
            for (uint32_t i = 0; i < zp.size(); i++) { blockIdx.x = i; k_witness_expand(zp.data(), plain.desc.data(), (uint32_t)zp.size(), plain_trace.data() + p * plain.trace_bytes, plain.sbox_in_off.data(), plain.sbox_tmpl.data(), sb); }
            const size_t bad = unsatisfied(c, z);
            reveal_bytes(msg, mask, L, revealed.data());                                                // the verifier's masking
            // the instance: the R = 0 circuit's, then the mask, revealed, then zero padding
            size_t ibad = 0, at = plain.raw_instance;
            for (size_t i = 0; i < plain.raw_instance; i++) ibad += z[i] != zp[i];
            for (size_t j = 0; j < mb; j++) for (int k = 0; k < 8; k++) ibad += z[at++] != ((mask[j] >> k) & 1);
            const size_t rev_z = at;
            for (size_t j = 0; j < L; j++) for (int k = 0; k < 8; k++) ibad += z[at++] != ((revealed[j] >> k) & 1);
            if (at != c.raw_instance) ibad++;
            for (; at < c.num_instance; at++) ibad += z[at] != 0;
            memcpy(want_region.data(), mask, mb);
            memcpy(want_region.data() + rev_at, revealed.data(), L);
            ibad += memcmp(tr + rv, want_region.data(), region) != 0;
            // one revealed bit flipped: exactly its product row; one mask bit at a revealed (non-zero) byte flipped: at least one row
            const size_t victim = (5 + 13 * p) % L;
            std::vector<uint8_t> zf(z);
            zf[rev_z + 8 * victim + 3] ^= 1;
            const size_t flip_rev = unsatisfied(c, zf);
            size_t shown = L;
            for (size_t i = 0; i < L; i++) if (revealed[i]) { shown = i; break; }
            size_t flip_mask = 1;
            if (shown < L) { zf = z; zf[plain.raw_instance + shown] ^= 1; flip_mask = unsatisfied(c, zf); }
            printf("%s proof %u mask %s: unsatisfied %zu, instance and region mismatches %zu, rows unsatisfied after a revealed-bit flip %zu, after a mask-bit flip %zu%s\n", name, p,
                   mask_name[2 * launch + p], bad, ibad, flip_rev, flip_mask, shown < L ? "" : " (nothing revealed: not flipped)");
            bad_total += (int)(bad + ibad) + (flip_rev != 1) + (flip_mask < 1);
        }
    }
}

int main() {
    for (int i = 0; i < 256; i++) sb[i] = aes_sbox_value((uint8_t)i);
    int bad_total = 0;
    run<4>(ECB, 16, 0, 0, 0, bad_total);
    run<4>(CTR, 1, 0, 1, 2, bad_total);
    run<4>(CTR, 17, 0, 1, 2, bad_total);
    run<6>(CBC, 32, 0, 0, 0, bad_total);
    run<8>(GCM, 17, 5, 0, 0, bad_total);
    run<8>(ECB, 64, 0, 2, 1, bad_total);
    printf("total bad %d\n", bad_total);
    return bad_total != 0;
}
