// tests/gcm_segment_keytag_trace_emu.cpp -- the trace of a GCM segment HEAD key with key_tag_blocks = T: k_aes_trace_gcm_seg, k_ghash_trace_seg and
// k_key_tag_trace of csrc/kernels_witness.cuh, k_commit_trace of csrc/kernels_digest.cuh, k_reveal_trace of csrc/kernels_reveal.cuh for the reveal shape and
// k_witness_expand, run lane by lane ON THE HOST: tests/test_gcm_segments_keytag_host.py builds this file, which includes the three kernel headers behind
// tests/lane_emu.h, with -fsanitize=address,undefined.  Shapes: head c = 1, A = 0, AES-128, T = 1; head c = 2, A = 5, AES-128, T = 2; head c = 1, A = 13,
// AES-256, T = 1; head c = 1, A = 5, AES-192, T = 1 with reveal.  Every head is segment 0 of a real record of two segments, as in tests/gcm_segment_trace_emu.cpp.  Two
// proofs with different keys, messages, ivs, aad and salts per launch; the message, key and header buffers hold exactly the bytes that exist, on the heap, and guard
// bytes lie behind the traces.  The kernels are launched as ProvingKeyImpl::launch_trace launches them: the segment kernels, the tag kernel at the circuit's key_tag_off
// over the circuit's stride, the reveal kernel last.
// Checked per shape: the circuit's header against the T = 0 circuit's (key_tag_off = that circuit's trace length rounded up to 16 = TRS_KT; T block strides more trace;
// the reveal region where the slots end; 128 T more instance bits behind com_out and ahead of the mask).  With every lane of the kernels run alone over traces
// prefilled with two different patterns: no byte has two writers, the guard bytes and the alignment padding have none, every byte of the tag slots has exactly one
// writing lane, and that lane is the tag kernel's, which writes nowhere else; with reveal every byte of the reveal region has its one writer, a reveal lane.  After the
// launch as the library makes it: the bytes ahead of the slots are the T = 0 key's trace, and with reveal the region behind the slots is the T = 0 reveal key's region.
// Per proof: every row of (A z) o (B z) = C z holds; the instance is One, what the host says for a head, zkaes_key_tag's bits, (the mask and revealed slices,) zero
// padding; ONE flipped tag bit leaves exactly one row unsatisfied.  No GPU: what the device adds is the launch.
#include "circuit.hpp"
#include "statement.hpp"
#include "trace_layout.h"
#include "../include/zkaes.h"
#include <array>
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
#define CHECK_RC(call) do { if ((call) != 0) { printf("%s: %s\n", #call, zkaes_last_error()); exit(1); } } while (0)

struct Launch {
    uint32_t nproofs, nb, na, len, alen, ntags; size_t kb, stride, seg_off, yout_off, hs, kt_off, rv_off, rhs;
    const uint8_t *msgs, *keys, *hdrs, *rhdrs;
    uint32_t aes_lanes() const { return nproofs * (uint32_t)(TRS_SLOTS(TRS_HEAD, nb) + 1); }
    uint32_t ghash_lanes() const { return nproofs * (uint32_t)(TRS_MULS(TRS_HEAD, na, nb) + 1) * 16; }
    uint32_t commit_lanes() const { return nproofs; }
    uint32_t tag_lanes() const { return nproofs * ntags; }
    uint32_t reveal_lanes() const { return nproofs * nb; }
};
enum { K_AES, K_GHASH, K_COMMIT, K_TAG, K_REVEAL };
template <int NK> static void lane(const Launch &l, int kernel, uint8_t *trace, uint32_t t) {
    blockIdx.x = t;
    if (kernel == K_AES) k_aes_trace_gcm_seg<NK>(trace, l.stride, l.msgs, l.keys, l.hdrs, l.nproofs, (uint32_t)TRS_HEAD, l.nb, l.na, l.len, l.alen, sb);
    else if (kernel == K_GHASH) k_ghash_trace_seg<NK>(trace, l.stride, l.nproofs, (uint32_t)TRS_HEAD, l.nb, l.na);
    else if (kernel == K_COMMIT) k_commit_trace(trace, l.stride, l.seg_off, l.yout_off, l.keys, (uint32_t)l.kb, l.hdrs, l.hs, l.nproofs, (uint32_t)TRS_HEAD, l.nb);
    else if (kernel == K_TAG) k_key_tag_trace<NK>(trace, l.stride, l.kt_off, l.keys, l.nproofs, l.ntags, sb);      // as gpu::key_tag_trace launches it: the circuit's stride and key_tag_off
    else k_reveal_trace(trace, l.stride, l.rv_off, l.msgs, l.rhdrs, l.rhs, l.hs, l.nproofs, l.nb, l.len);
}
static uint32_t lanes_of(const Launch &l, int kernel) {
    return kernel == K_AES ? l.aes_lanes() : kernel == K_GHASH ? l.ghash_lanes() : kernel == K_COMMIT ? l.commit_lanes() : kernel == K_TAG ? l.tag_lanes() : l.reveal_lanes();
}
template <int NK> static void launch_all(const Launch &l, uint8_t *trace, bool reveal) {
    for (int k = K_AES; k <= K_COMMIT; k++) for (uint32_t t = 0; t < lanes_of(l, k) + 3; t++) lane<NK>(l, k, trace, t);
    if (l.ntags) for (uint32_t t = 0; t < l.tag_lanes() + 3; t++) lane<NK>(l, K_TAG, trace, t);
    if (reveal) for (uint32_t t = 0; t < l.reveal_lanes() + 3; t++) lane<NK>(l, K_REVEAL, trace, t);
}
static void put32(uint8_t *p, uint32_t v) { for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (24 - 8 * i)); }

// a head of c data blocks under A bytes of aad with T tag blocks, R = reveal
template <int NK>
static void run(size_t c, size_t A, size_t T, int R, int &bad_total) {
    const size_t kb = 4 * NK, len = 16 * c, nb = c, na = (A + 15) / 16, mb = mask_bytes(len), n = 2, L = 16 * c + 9;      // the record around the segment
    const Circuit cc = compile_aes_gcm_segment_circuit(TRS_HEAD, c, A, 8 * kb, R, T), plain = compile_aes_gcm_segment_circuit(TRS_HEAD, c, A, 8 * kb, R, 0),
                  bare = compile_aes_gcm_segment_circuit(TRS_HEAD, c, A, 8 * kb, 0, 0);
    char name[96];
    snprintf(name, sizeof name, "NK=%d head c=%zu A=%zu T=%zu R=%d", NK, c, A, T, R);
    const size_t gcm = TRS_GCM(NK, TRS_HEAD, nb), sg = gcm + TRS_SEG(TRS_HEAD, na, nb), n_mul = TRS_MULS(TRS_HEAD, na, nb), slot = TRK_BLOCK_STRIDE(NK);
    const size_t kt = TRS_KT(NK, TRS_HEAD, na, nb), rv = R ? TRS_KT_RV(NK, TRS_HEAD, na, nb, T) : 0, region = R ? TRV_REGION_BYTES(len) : 0, rev_at = TRV_REVEALED(len);
    // a block of one key size: rows and witnesses of DESIGN.md 9e's table
    const size_t rows_per = NK == 4 ? 148016 : NK == 6 ? 177680 : 207344, wits_per = NK == 4 ? 147760 : NK == 6 ? 177424 : 207088;
    if (cc.kind != CIRCUIT_AES_GCM_SEG || cc.seg_role != TRS_HEAD || cc.seg_off != sg || bare.trace_bytes != TRS_BYTES(NK, TRS_HEAD, na, nb) || cc.key_tag_blocks != T || plain.key_tag_blocks != 0 ||
        plain.key_tag_off != 0 || cc.key_tag_off != kt || kt != (bare.trace_bytes + 15) / 16 * 16 || kt % 16 || cc.trace_bytes % 16 || cc.trace_bytes != TRS_KT_RV_BYTES(NK, TRS_HEAD, na, nb, T, R, len) ||
        cc.trace_bytes != (R ? rv + region : kt + T * slot) || (R && (cc.reveal_off != rv || rv != kt + T * slot || plain.reveal_off != TRS_RV(NK, TRS_HEAD, na, nb))) || (!R && cc.reveal_off != 0) ||
        cc.message_bytes != len || cc.raw_instance != plain.raw_instance + 128 * T || cc.raw_constraints != plain.raw_constraints + rows_per * T || cc.raw_witness != plain.raw_witness + wits_per * T ||
        mode_header_bytes(cc) != TRS_HDR_BYTES(A) || reveal_mask_bytes(cc) != (R ? mb : 0)) {
        printf("%s: circuit header is off\n", name); bad_total++;
    }
    const uint32_t nproofs = 2;
    const size_t hs = TRS_HDR_BYTES(A), rhs = hs + (R ? mb : 0), stride = cc.trace_bytes, total = stride * nproofs + 64;
    std::unique_ptr<uint8_t[]> msgs(new uint8_t[len * nproofs]), keys(new uint8_t[kb * nproofs]), hdrs(new uint8_t[hs * nproofs]), rhdrs(new uint8_t[rhs * nproofs]);      // exactly the bytes that exist
    std::vector<std::vector<uint8_t>> rec_ct(nproofs), coms(nproofs), aads(nproofs), ivs(nproofs), rec_mask(nproofs), rec_revealed(nproofs), key_tags(nproofs);
    srand(9200 + 100 * NK + 10 * (unsigned)T + (unsigned)c + (unsigned)A);
    for (uint32_t p = 0; p < nproofs; p++) {
        std::unique_ptr<uint8_t[]> rec(new uint8_t[L]), aad(new uint8_t[A ? A : 1]);
        uint8_t iv[12], salts[16], tag[16], lenblk[16];
        for (size_t i = 0; i < L; i++) rec[i] = (uint8_t)(rand() | 1);
        for (size_t i = 0; i < A; i++) aad[i] = (uint8_t)rand();
        for (auto &x : iv) x = (uint8_t)rand();
        for (auto &x : salts) x = (uint8_t)rand();
        uint8_t *key = keys.get() + kb * p;
        for (size_t i = 0; i < kb; i++) key[i] = (uint8_t)rand();
        rec_ct[p].resize(L); coms[p].resize(32 * (n - 1)); aads[p].assign(aad.get(), aad.get() + A); ivs[p].assign(iv, iv + 12); key_tags[p].resize(16 * T);
        CHECK_RC(zkaes_gcm_encrypt_ks(rec.get(), L, key, kb, iv, A ? aad.get() : nullptr, A, rec_ct[p].data(), tag));
        CHECK_RC(zkaes_key_tag(key, kb, T, key_tags[p].data()));
        uint8_t ys[16];
        size_t n_seg = 0;
        CHECK_RC(zkaes_gcm_boundaries(rec.get(), L, key, kb, iv, A ? aad.get() : nullptr, A, c, ys, 16, &n_seg));
        if (n_seg != n) { printf("%s: the record has %zu segments, not %zu\n", name, n_seg, n); bad_total++; }
        CHECK_RC(zkaes_gcm_commit(key, kb, ys, salts, coms[p].data()));
        for (int i = 0; i < 8; i++) { lenblk[i] = (uint8_t)((uint64_t)(8 * A) >> (56 - 8 * i)); lenblk[8 + i] = (uint8_t)((uint64_t)(8 * L) >> (56 - 8 * i)); }
        rec_mask[p].assign(mask_bytes(L), 0);
        for (size_t i = 0; i < L; i++) if (p == 0 ? i % 2 == 0 : (rand() & 1)) rec_mask[p][i / 8] |= (uint8_t)(1u << (i % 8));
        for (size_t i : {(size_t)0, len - 1}) rec_mask[p][i / 8] |= (uint8_t)(1u << (i % 8));
        rec_revealed[p].resize(L);
        CHECK_RC(zkaes_reveal_bytes(rec.get(), L, rec_mask[p].data(), rec_mask[p].size(), rec_revealed[p].data()));
        memcpy(msgs.get() + len * p, rec.get(), len);
        uint8_t *h = hdrs.get() + hs * p;
        memset(h, 0, hs);
        memcpy(h + TRS_HDR_IV, iv, 12);
        put32(h + TRS_HDR_CTR0, 2);
        memcpy(h + TRS_HDR_SALT_OUT, salts, 16);
        memcpy(h + TRS_HDR_LEN, lenblk, 16);
        if (A) memcpy(h + TRS_HDR_AAD, aad.get(), A);
        memcpy(rhdrs.get() + rhs * p, h, hs);
        if (R) memcpy(rhdrs.get() + rhs * p + TRS_HDR_MASK(A), chunk_mask_slice(rec_mask[p].data(), 0, 16 * c), mb);
    }
    const size_t yout_off = gcm + TR_GCM_MUL0(na, nb) + (n_mul - 1) * TR_GCM_MUL_STRIDE + TR_GCM_MUL_Y;
    Launch l{nproofs, (uint32_t)nb, (uint32_t)na, (uint32_t)len, (uint32_t)A, (uint32_t)T, kb, stride, sg, yout_off, hs, cc.key_tag_off, cc.reveal_off, rhs, msgs.get(), keys.get(), hdrs.get(), rhdrs.get()};
    // ---- who writes what: every lane of every kernel alone, over two prefill patterns (a byte is written iff it leaves either pattern; Y_out, which the com_out lane
    // reads, holds random bytes in both, as in tests/gcm_segment_trace_emu.cpp)
    std::vector<uint32_t> writers(total, 0), tag_writers(total, 0), reveal_writers(total, 0);
    size_t lane_bad = 0;
    std::vector<uint8_t> fill_a(total, 0xAA), fill_b(total, 0x55);
    for (uint32_t p = 0; p < nproofs; p++) for (int i = 0; i < 16; i++) { fill_a[p * stride + yout_off + i] = (uint8_t)rand(); fill_b[p * stride + yout_off + i] = (uint8_t)rand(); }
    auto in_slots = [&](size_t i) { return i < stride * nproofs && i % stride >= kt && i % stride < kt + T * slot; };
    auto alone = [&](int kernel, uint32_t t, uint32_t lanes) {
        std::vector<uint8_t> a(fill_a), b(fill_b);
        for (std::vector<uint8_t> *tr : {&a, &b}) lane<NK>(l, kernel, tr->data(), t);
        size_t wrote = 0, inside = 0;
        for (size_t i = 0; i < total; i++) if (a[i] != fill_a[i] || b[i] != fill_b[i]) { writers[i]++; wrote++; inside += in_slots(i); if (kernel == K_TAG) tag_writers[i]++; if (kernel == K_REVEAL) reveal_writers[i]++; }
        if (t >= lanes && wrote) { printf("%s: a lane of kernel %d beyond the grid wrote to the trace\n", name, kernel); lane_bad++; }
        if (kernel != K_TAG && inside) { printf("%s: lane %u of kernel %d wrote %zu bytes of the tag slots\n", name, t, kernel, inside); lane_bad++; }
        if (kernel == K_TAG && t < lanes && (wrote != slot || inside != slot)) { printf("%s: tag lane %u wrote %zu bytes, %zu of them inside the slots (want %zu)\n", name, t, wrote, inside, slot); lane_bad++; }
    };
    for (int k = K_AES; k <= (R ? K_REVEAL : K_TAG); k++) for (uint32_t t = 0; t < lanes_of(l, k) + 3; t++) alone(k, t, lanes_of(l, k));
    size_t two_writers = 0, guard_writers = 0, slot_bad = 0, tag_elsewhere = 0, padding_written = 0, region_bad = 0;
    for (size_t i = 0; i < total; i++) {
        if (i >= stride * nproofs) { guard_writers += writers[i] != 0; continue; }
        two_writers += writers[i] > 1;
        const size_t o = i % stride;
        if (in_slots(i)) slot_bad += writers[i] != 1 || tag_writers[i] != 1;                                // one writing lane per byte of the slots, the tag kernel's
        else tag_elsewhere += tag_writers[i] != 0;                                                          // and none elsewhere from it
        if (o >= bare.trace_bytes && o < kt) padding_written += writers[i] != 0;                            // the alignment bytes between the compression slots and slot 0
        if (R && o >= rv) region_bad += writers[i] != 1 || reveal_writers[i] != 1;
    }
    printf("%s: bytes with two writers %zu, guard bytes written %zu, alignment bytes written %zu, tag slot bytes without their one tag lane %zu, bytes elsewhere the tag kernel wrote %zu, "
           "reveal region bytes without their one writer %zu, lane faults %zu\n", name, two_writers, guard_writers, padding_written, slot_bad, tag_elsewhere, region_bad, lane_bad);
    bad_total += (two_writers != 0) + (guard_writers != 0) + (padding_written != 0) + (slot_bad != 0) + (tag_elsewhere != 0) + (region_bad != 0) + (lane_bad != 0);
    // ---- the launch as the library makes it; the bytes ahead of the slots are the T = 0 head's trace, the reveal region behind them the T = 0 reveal head's
    std::vector<uint8_t> trace(total, 0xAA), plain_trace(plain.trace_bytes * nproofs + 64, 0xAA);
    launch_all<NK>(l, trace.data(), R != 0);
    Launch lp = l;
    lp.stride = plain.trace_bytes; lp.ntags = 0; lp.kt_off = 0; lp.rv_off = plain.reveal_off;
    launch_all<NK>(lp, plain_trace.data(), R != 0);
    size_t differs = 0, region_differs = 0;
    for (uint32_t p = 0; p < nproofs; p++) {
        differs += memcmp(trace.data() + p * stride, plain_trace.data() + p * plain.trace_bytes, bare.trace_bytes) != 0;
        if (R) region_differs += memcmp(trace.data() + p * stride + rv, plain_trace.data() + p * plain.trace_bytes + plain.reveal_off, region) != 0;
    }
    for (size_t i = stride * nproofs; i < total; i++) if (trace[i] != 0xAA) { printf("%s: write past the traces\n", name); bad_total++; break; }
    if (differs) { printf("%s: %zu proofs whose bytes ahead of the tag slots differ from the T = 0 trace\n", name, differs); bad_total++; }
    if (region_differs) { printf("%s: %zu proofs whose reveal region behind the tag slots differs from the T = 0 key's\n", name, region_differs); bad_total++; }
    for (uint32_t p = 0; p < nproofs; p++) {
        const uint8_t *tr = trace.data() + p * stride, *mask = rhdrs.get() + rhs * p + hs, *revealed = rec_revealed[p].data();
        std::vector<uint8_t> z(cc.num_variables());
        for (uint32_t i = 0; i < z.size(); i++) { blockIdx.x = i; k_witness_expand(z.data(), cc.desc.data(), (uint32_t)z.size(), tr, cc.sbox_in_off.data(), cc.sbox_tmpl.data(), sb); }
        const size_t bad = unsatisfied(cc, z);
        // the instance: One, iv, ctr0, (aad), the ciphertext slice, com_out, the key tag, (the mask slice, the revealed slice,) zero padding
        size_t ibad = z[0] != 1, at = 1;
        auto expect = [&](const uint8_t *d, size_t nbytes) { for (size_t i = 0; i < nbytes; i++) for (int k = 0; k < 8; k++) ibad += z[at++] != ((d[i] >> k) & 1); };
        uint8_t ctr0[4];
        put32(ctr0, 2);
        expect(ivs[p].data(), 12);
        expect(ctr0, 4);
        if (A) expect(aads[p].data(), A);
        expect(rec_ct[p].data(), len);
        expect(coms[p].data(), 32);
        if (at != bare.raw_instance) ibad++;
        const size_t tag_at = at;
        expect(key_tags[p].data(), 16 * T);
        if (R) { expect(mask, mb); expect(revealed, len); }
        if (at != cc.raw_instance) ibad++;
        for (; at < cc.num_instance; at++) ibad += z[at] != 0;
        // the slots themselves end in the tag: S_Nr of slot t = tag_t, and the slot's "message" field is D_t
        for (size_t t = 0; t < T; t++) {
            uint8_t d[16];
            aes_key_tag_block(t, d);
            ibad += memcmp(tr + TRK_KT_SLOT(NK, bare.trace_bytes, t) + TRK_BL_CT(NK), key_tags[p].data() + 16 * t, 16) != 0;
            ibad += memcmp(tr + TRK_KT_SLOT(NK, bare.trace_bytes, t), d, 16) != 0;
        }
        if (R) {
            std::vector<uint8_t> want_region(region, 0);
            memcpy(want_region.data(), mask, mb);
            memcpy(want_region.data() + rev_at, revealed, len);
            ibad += memcmp(tr + rv, want_region.data(), region) != 0;
        }
        // ONE flipped tag bit: exactly the row that ties that input to S_Nr's bit
        std::vector<uint8_t> zf(z);
        zf[tag_at + (37 + 61 * p) % (128 * T)] ^= 1;
        const size_t flip_tag = unsatisfied(cc, zf);
        printf("%s proof %u: unsatisfied %zu, instance and slot mismatches %zu, rows unsatisfied after one flipped tag bit %zu\n", name, p, bad, ibad, flip_tag);
        bad_total += (int)(bad + ibad) + (flip_tag != 1);
    }
}

int main() {
    for (int i = 0; i < 256; i++) sb[i] = aes_sbox_value((uint8_t)i);
    int bad_total = 0;
    run<4>(1, 0, 1, 0, bad_total);
    run<4>(2, 5, 2, 0, bad_total);
    run<8>(1, 13, 1, 0, bad_total);
    run<6>(1, 5, 1, 1, bad_total);
    printf("total bad %d\n", bad_total);
    return bad_total != 0;
}
