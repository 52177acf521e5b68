// tests/gcm_segment_reveal_trace_emu.cpp -- the trace of a GCM segment key with reveal = 1: k_aes_trace_gcm_seg and k_ghash_trace_seg of
// csrc/kernels_witness.cuh, k_commit_trace of csrc/kernels_digest.cuh, k_reveal_trace of csrc/kernels_reveal.cuh behind them and k_witness_expand, run lane by lane ON THE
// HOST: tests/test_gcm_segments_reveal_host.py builds this file, which includes the three kernel headers behind tests/lane_emu.h, with
// -fsanitize=address,undefined.  Shapes: head (A = 13, c = 1), mid (c = 1), tail (Lt = 7, c = 1); head (A = 0, c = 2), tail (Lt = 17, c = 2); an AES-256 mid (c = 1).
// Every shape is a segment of a real record, as in tests/gcm_segment_trace_emu.cpp -- a head is segment 0 of two, a mid segment 1 of three, a tail segment 1 of two --
// under ONE mask over the record, every second byte of it open and then some, so that the segment is proven under its slice (statement.hpp chunk_mask_slice) and the
// instance is compared with the host-only entries and the host's masking.  Two proofs with different keys, messages, ivs, aad, salts and masks per launch; no message
// byte is zero (a hidden byte and a revealed zero byte differ in the mask alone, DESIGN.md 9i, so the flips below would not show); the message, key and header buffers
// hold exactly the bytes that exist, on the heap -- the segment kernels read headers of 80 + A bytes, the reveal kernel headers of 80 + A + ceil(len / 8) with its
// mask_off = 80 + A, as launch_trace hands them over -- and guard bytes lie behind the traces.
// Checked per shape: the circuit's header against the R = 0 circuit's (the region's offset = that circuit's trace length rounded up to 16; 8 ceil(len / 8) + 8 len more
// instance bits, 16 ceil(len / 8) + 15 len more rows, no more witnesses).  With every lane of the four kernels run alone over traces prefilled with two different
// patterns: no byte of the traces has two writers, the guard bytes and the alignment padding have none, every byte of the reveal region has exactly one, and no reveal
// lane writes ahead of reveal_off or beyond the grid.  After the launch as the library makes it: the bytes ahead of the region are the R = 0 key's trace.  Per proof:
// every row of (A z) o (B z) = C z holds; the instance is One, what the host says for the role, the mask slice, revealed from the host's masking, zero padding; a
// flipped mask bit, a flipped revealed bit and -- for a tail whose length is no multiple of 8 -- a mask bit at position >= Lt handed to the KERNEL each leave at least
// one row unsatisfied.  No GPU: what the device adds is the launch.
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
static const char *role_name[3] = {"head", "mid", "tail"};
#define CHECK_RC(call) do { if ((call) != 0) { printf("%s: %s\n", #call, zkaes_last_error()); exit(1); } } while (0)

struct Launch {
    int role; uint32_t nproofs, nb, na, len, alen; size_t kb, stride, seg_off, yout_off, hs, rv_off, rhs;
    const uint8_t *msgs, *keys, *hdrs, *rhdrs;
    uint32_t aes_lanes() const { return nproofs * (uint32_t)(TRS_SLOTS(role, nb) + 1); }
    uint32_t ghash_lanes() const { return nproofs * (uint32_t)(TRS_MULS(role, na, nb) + 1) * 16; }
    uint32_t commit_lanes() const { return nproofs * (role == TRS_MID ? 2u : 1u); }
    uint32_t reveal_lanes() const { return nproofs * nb; }
};
template <int NK> static void aes_lane(const Launch &l, uint8_t *trace, uint32_t t) { blockIdx.x = t; k_aes_trace_gcm_seg<NK>(trace, l.stride, l.msgs, l.keys, l.hdrs, l.nproofs, (uint32_t)l.role, l.nb, l.na, l.len, l.alen, sb); }
template <int NK> static void ghash_lane(const Launch &l, uint8_t *trace, uint32_t t) { blockIdx.x = t; k_ghash_trace_seg<NK>(trace, l.stride, l.nproofs, (uint32_t)l.role, l.nb, l.na); }
static void commit_lane(const Launch &l, uint8_t *trace, uint32_t t) { blockIdx.x = t; k_commit_trace(trace, l.stride, l.seg_off, l.yout_off, l.keys, (uint32_t)l.kb, l.hdrs, l.hs, l.nproofs, (uint32_t)l.role, l.nb); }
// the reveal kernel as launch_trace launches it for a segment key: the header stride holds the mask behind the 80 + A bytes, mask_off = 80 + A
static void reveal_lane(const Launch &l, uint8_t *trace, uint32_t t) { blockIdx.x = t; k_reveal_trace(trace, l.stride, l.rv_off, l.msgs, l.rhdrs, l.rhs, l.hs, l.nproofs, l.nb, l.len); }
template <int NK> static void launch_all(const Launch &l, uint8_t *trace, bool reveal) {
    for (uint32_t t = 0; t < l.aes_lanes() + 3; t++) aes_lane<NK>(l, trace, t);
    for (uint32_t t = 0; t < l.ghash_lanes() + 3; t++) ghash_lane<NK>(l, trace, t);
    for (uint32_t t = 0; t < l.commit_lanes() + 3; t++) commit_lane(l, trace, t);
    if (reveal) for (uint32_t t = 0; t < l.reveal_lanes() + 3; t++) reveal_lane(l, trace, t);
}
static void put32(uint8_t *p, uint32_t v) { for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (24 - 8 * i)); }

// role: the shape's; c: data blocks per segment; units: c (head, mid) or Lt (tail); A: the record's aad
template <int NK>
static void run(int role, size_t c, size_t units, size_t A, int &bad_total) {
    const size_t kb = 4 * NK, len = role == TRS_TAIL ? units : 16 * c, nb = (len + 15) / 16, seg_a = role == TRS_HEAD ? A : 0, na = (seg_a + 15) / 16, mb = mask_bytes(len);
    const size_t s = role == TRS_HEAD ? 0 : 1, n = role == TRS_MID ? 3 : 2, L = role == TRS_HEAD ? 16 * c + 9 : role == TRS_MID ? 32 * c + 5 : 16 * c + units;      // the record around the segment
    const Circuit cc = compile_aes_gcm_segment_circuit(role, units, seg_a, 8 * kb, 1), plain = compile_aes_gcm_segment_circuit(role, units, seg_a, 8 * kb, 0);
    char name[96];
    snprintf(name, sizeof name, "NK=%d %s c=%zu units=%zu A=%zu", NK, role_name[role], c, units, A);
    const size_t gcm = TRS_GCM(NK, role, nb), sg = gcm + TRS_SEG(role, na, nb), n_mul = TRS_MULS(role, na, nb);
    const size_t rv = TRS_RV(NK, role, na, nb), region = TRV_REGION_BYTES(len), rev_at = TRV_REVEALED(len);
    if (cc.kind != CIRCUIT_AES_GCM_SEG || cc.seg_role != role || cc.seg_off != sg || plain.trace_bytes != TRS_BYTES(NK, role, na, nb) || cc.reveal != 1 || plain.reveal != 0 || plain.reveal_off != 0 ||
        cc.reveal_off != rv || rv != (plain.trace_bytes + 15) / 16 * 16 || cc.trace_bytes != rv + region || cc.trace_bytes != TRS_RV_BYTES(NK, role, na, nb, 1, len) || cc.trace_bytes % 16 ||
        cc.message_bytes != len || cc.raw_instance != plain.raw_instance + 8 * mb + 8 * len || cc.raw_constraints != plain.raw_constraints + 16 * mb + 15 * len || cc.raw_witness != plain.raw_witness ||
        mode_header_bytes(cc) != TRS_HDR_BYTES(seg_a) || reveal_mask_bytes(cc) != mb || reveal_mask_bytes(plain) != 0 || TRS_HDR_RV_BYTES(seg_a, 1, len) != TRS_HDR_BYTES(seg_a) + mb) {
        printf("%s: circuit header is off\n", name); bad_total++;
    }
    const uint32_t nproofs = 2;
    const size_t hs = TRS_HDR_BYTES(seg_a), rhs = hs + mb, stride = cc.trace_bytes, total = stride * nproofs + 64;
    std::unique_ptr<uint8_t[]> msgs(new uint8_t[len * nproofs]), keys(new uint8_t[kb * nproofs]), hdrs(new uint8_t[hs * nproofs]), rhdrs(new uint8_t[rhs * nproofs]);      // exactly the bytes that exist
    std::vector<std::vector<uint8_t>> rec_ct(nproofs), coms(nproofs), aads(nproofs), ivs(nproofs), rec_mask(nproofs), rec_revealed(nproofs);
    std::vector<std::array<uint8_t, 16>> tags(nproofs), lenblks(nproofs);
    srand(9100 + 100 * NK + 10 * (unsigned)role + (unsigned)units + (unsigned)A);
    for (uint32_t p = 0; p < nproofs; p++) {
        std::unique_ptr<uint8_t[]> rec(new uint8_t[L]), aad(new uint8_t[A ? A : 1]);
        uint8_t iv[12], salts[32];
        for (size_t i = 0; i < L; i++) rec[i] = (uint8_t)(rand() | 1);                                  // no zero byte
        for (size_t i = 0; i < A; i++) aad[i] = (uint8_t)rand();
        for (auto &x : iv) x = (uint8_t)rand();
        for (auto &x : salts) x = (uint8_t)rand();
        uint8_t *key = keys.get() + kb * p;
        for (size_t i = 0; i < kb; i++) key[i] = (uint8_t)rand();
        rec_ct[p].resize(L); coms[p].resize(32 * (n - 1)); aads[p].assign(aad.get(), aad.get() + A); ivs[p].assign(iv, iv + 12);
        CHECK_RC(zkaes_gcm_encrypt_ks(rec.get(), L, key, kb, iv, A ? aad.get() : nullptr, A, rec_ct[p].data(), tags[p].data()));
        std::unique_ptr<uint8_t[]> ys(new uint8_t[16 * (n - 1)]);
        size_t n_seg = 0;
        CHECK_RC(zkaes_gcm_boundaries(rec.get(), L, key, kb, iv, A ? aad.get() : nullptr, A, c, ys.get(), 16 * (n - 1), &n_seg));
        if (n_seg != n) { printf("%s: the record has %zu segments, not %zu\n", name, n_seg, n); bad_total++; }
        for (size_t b = 0; b + 1 < n; b++) CHECK_RC(zkaes_gcm_commit(key, kb, ys.get() + 16 * b, salts + 16 * b, coms[p].data() + 32 * b));
        for (int i = 0; i < 8; i++) { lenblks[p][i] = (uint8_t)((uint64_t)(8 * A) >> (56 - 8 * i)); lenblks[p][8 + i] = (uint8_t)((uint64_t)(8 * L) >> (56 - 8 * i)); }
        // ONE mask over the record: proof 0 opens every second byte, proof 1 a random half; both open the segment's first and last byte, so the lane and segment edges show
        rec_mask[p].assign(mask_bytes(L), 0);
        for (size_t i = 0; i < L; i++) if (p == 0 ? i % 2 == 0 : (rand() & 1)) rec_mask[p][i / 8] |= (uint8_t)(1u << (i % 8));
        for (size_t i : {16 * c * s, 16 * c * s + len - 1}) rec_mask[p][i / 8] |= (uint8_t)(1u << (i % 8));
        rec_revealed[p].resize(L);
        CHECK_RC(zkaes_reveal_bytes(rec.get(), L, rec_mask[p].data(), rec_mask[p].size(), rec_revealed[p].data()));
        memcpy(msgs.get() + len * p, rec.get() + 16 * c * s, len);
        uint8_t *h = hdrs.get() + hs * p;
        memset(h, 0, hs);
        memcpy(h + TRS_HDR_IV, iv, 12);
        put32(h + TRS_HDR_CTR0, (uint32_t)(2 + s * c));
        if (s) { memcpy(h + TRS_HDR_YIN, ys.get() + 16 * (s - 1), 16); memcpy(h + TRS_HDR_SALT_IN, salts + 16 * (s - 1), 16); }
        if (s + 1 < n) memcpy(h + TRS_HDR_SALT_OUT, salts + 16 * s, 16);
        memcpy(h + TRS_HDR_LEN, lenblks[p].data(), 16);
        if (seg_a) memcpy(h + TRS_HDR_AAD, aad.get(), seg_a);
        memcpy(rhdrs.get() + rhs * p, h, hs);
        memcpy(rhdrs.get() + rhs * p + TRS_HDR_MASK(seg_a), chunk_mask_slice(rec_mask[p].data(), s, 16 * c), mb);      // the segment's slice: the statement layer's one definition
    }
    const size_t yout_off = gcm + TR_GCM_MUL0(na, nb) + (n_mul - 1) * TR_GCM_MUL_STRIDE + TR_GCM_MUL_Y;
    Launch l{role, nproofs, (uint32_t)nb, (uint32_t)na, (uint32_t)len, (uint32_t)seg_a, kb, stride, sg, yout_off, hs, rv, rhs, msgs.get(), keys.get(), hdrs.get(), rhdrs.get()};
    // ---- who writes what: every lane of the four kernels alone, over two prefill patterns (a byte is written iff it leaves either pattern; Y_out, which a com_out
    // lane reads, holds random bytes in both, as in tests/gcm_segment_trace_emu.cpp)
    std::vector<uint32_t> writers(total, 0);
    size_t lane_bad = 0;
    std::vector<uint8_t> fill_a(total, 0xAA), fill_b(total, 0x55);
    for (uint32_t p = 0; p < nproofs; p++) for (int i = 0; i < 16; i++) { fill_a[p * stride + yout_off + i] = (uint8_t)rand(); fill_b[p * stride + yout_off + i] = (uint8_t)rand(); }
    auto alone = [&](int kernel, uint32_t t, uint32_t lanes) {
        std::vector<uint8_t> a(fill_a), b(fill_b);
        for (std::vector<uint8_t> *tr : {&a, &b}) {
            if (kernel == 0) aes_lane<NK>(l, tr->data(), t); else if (kernel == 1) ghash_lane<NK>(l, tr->data(), t); else if (kernel == 2) commit_lane(l, tr->data(), t); else reveal_lane(l, tr->data(), t);
        }
        size_t wrote = 0, ahead = 0, inside = 0;
        for (size_t i = 0; i < total; i++) if (a[i] != fill_a[i] || b[i] != fill_b[i]) { writers[i]++; wrote++; ahead += i >= stride * nproofs || i % stride < rv; inside += i < stride * nproofs && i % stride >= rv; }
        if (t >= lanes && wrote) { printf("%s: a lane of kernel %d beyond the grid wrote to the trace\n", name, kernel); lane_bad++; }
        if (kernel != 3 && inside) { printf("%s: lane %u of kernel %d wrote %zu bytes of the reveal region\n", name, t, kernel, inside); lane_bad++; }
        const size_t want = 18 + (t % nb == nb - 1 ? rev_at - 2 * nb : 0);                              // 16 revealed bytes, 2 mask bytes, and the last lane's mask padding
        if (kernel == 3 && t < lanes && (wrote != want || ahead)) { printf("%s: reveal lane %u wrote %zu bytes (want %zu), %zu of them ahead of reveal_off\n", name, t, wrote, want, ahead); lane_bad++; }
    };
    for (uint32_t t = 0; t < l.aes_lanes() + 3; t++) alone(0, t, l.aes_lanes());
    for (uint32_t t = 0; t < l.ghash_lanes() + 3; t++) alone(1, t, l.ghash_lanes());
    for (uint32_t t = 0; t < l.commit_lanes() + 3; t++) alone(2, t, l.commit_lanes());
    for (uint32_t t = 0; t < l.reveal_lanes() + 3; t++) alone(3, t, l.reveal_lanes());
    size_t two_writers = 0, guard_writers = 0, region_unwritten = 0, padding_written = 0;
    for (size_t i = 0; i < total; i++) {
        if (i >= stride * nproofs) { guard_writers += writers[i] != 0; continue; }
        two_writers += writers[i] > 1;
        const size_t o = i % stride;
        if (o >= rv) region_unwritten += writers[i] != 1;                                               // mask, its zero padding, revealed, its zero padding: one writer each
        else if (o >= plain.trace_bytes) padding_written += writers[i] != 0;                            // the alignment bytes between the compression slots and the region
    }
    printf("%s: bytes with two writers %zu, guard bytes written %zu, alignment bytes written %zu, reveal region bytes without their one writer %zu, lane faults %zu\n", name, two_writers, guard_writers,
           padding_written, region_unwritten, lane_bad);
    bad_total += (two_writers != 0) + (guard_writers != 0) + (padding_written != 0) + (region_unwritten != 0) + (lane_bad != 0);
    // ---- the launch as the library makes it; the bytes ahead of the region are the R = 0 key's trace
    std::vector<uint8_t> trace(total, 0xAA), plain_trace(plain.trace_bytes * nproofs + 64, 0xAA);
    launch_all<NK>(l, trace.data(), true);
    Launch lp = l;
    lp.stride = plain.trace_bytes;
    launch_all<NK>(lp, plain_trace.data(), false);
    size_t differs = 0;
    for (uint32_t p = 0; p < nproofs; p++) differs += memcmp(trace.data() + p * stride, plain_trace.data() + p * plain.trace_bytes, plain.trace_bytes) != 0;
    for (size_t i = stride * nproofs; i < total; i++) if (trace[i] != 0xAA) { printf("%s: write past the traces\n", name); bad_total++; break; }
    if (differs) { printf("%s: %zu proofs whose bytes ahead of the reveal region differ from the R = 0 trace\n", name, differs); bad_total++; }
    for (uint32_t p = 0; p < nproofs; p++) {
        const uint8_t *tr = trace.data() + p * stride, *mask = rhdrs.get() + rhs * p + hs, *revealed = rec_revealed[p].data() + 16 * c * s;
        std::vector<uint8_t> z(cc.num_variables());
        auto expand = [&](const uint8_t *from, std::vector<uint8_t> &into) {
            for (uint32_t i = 0; i < into.size(); i++) { blockIdx.x = i; k_witness_expand(into.data(), cc.desc.data(), (uint32_t)into.size(), from, cc.sbox_in_off.data(), cc.sbox_tmpl.data(), sb); }
        };
        expand(tr, z);
        const size_t bad = unsatisfied(cc, z);
        // the instance: One, iv, ctr0, (aad), the ciphertext slice, (length block, tag), (com_in), (com_out), the mask slice, the revealed slice, zero padding
        size_t ibad = z[0] != 1, at = 1;
        auto expect = [&](const uint8_t *d, size_t nbytes) { for (size_t i = 0; i < nbytes; i++) for (int k = 0; k < 8; k++) ibad += z[at++] != ((d[i] >> k) & 1); };
        uint8_t ctr0[4];
        put32(ctr0, (uint32_t)(2 + s * c));
        expect(ivs[p].data(), 12);
        expect(ctr0, 4);
        if (seg_a) expect(aads[p].data(), seg_a);
        expect(rec_ct[p].data() + 16 * c * s, len);
        if (role == TRS_TAIL) { expect(lenblks[p].data(), 16); expect(tags[p].data(), 16); }
        if (role != TRS_HEAD) expect(coms[p].data() + 32 * (s - 1), 32);
        if (role != TRS_TAIL) expect(coms[p].data() + 32 * s, 32);
        if (at != plain.raw_instance) ibad++;
        const size_t mask_at = at;
        expect(mask, mb);
        const size_t rev_z = at;
        expect(revealed, len);
        if (at != cc.raw_instance) ibad++;
        for (; at < cc.num_instance; at++) ibad += z[at] != 0;
        // the region itself: mask, zeros, revealed, zeros
        std::vector<uint8_t> want_region(region, 0);
        memcpy(want_region.data(), mask, mb);
        memcpy(want_region.data() + rev_at, revealed, len);
        ibad += memcmp(tr + rv, want_region.data(), region) != 0;
        // a flipped mask bit (no message byte is zero: an opened byte hidden, or a hidden byte opened, breaks a product row), a flipped revealed bit (exactly its row)
        const size_t victim = (5 + 13 * p) % len;
        std::vector<uint8_t> zf(z);
        zf[mask_at + victim] ^= 1;
        const size_t flip_mask = unsatisfied(cc, zf);
        zf = z; zf[rev_z + 8 * victim + 3] ^= 1;
        const size_t flip_rev = unsatisfied(cc, zf);
        // a mask bit at position >= Lt handed to the kernel: stored as it came, and the row that pins it is unsatisfied
        size_t beyond = 1;
        if (len % 8) {
            std::vector<uint8_t> hb(rhdrs.get(), rhdrs.get() + rhs * nproofs), tb(trace);
            hb[rhs * p + hs + len / 8] |= (uint8_t)(1u << (len % 8));
            Launch lb = l;
            lb.rhdrs = hb.data();
            for (uint32_t t = 0; t < lb.reveal_lanes(); t++) reveal_lane(lb, tb.data(), t);
            std::vector<uint8_t> zb(cc.num_variables());
            expand(tb.data() + p * stride, zb);
            beyond = unsatisfied(cc, zb);
        }
        printf("%s proof %u: unsatisfied %zu, instance and region mismatches %zu, rows unsatisfied after a mask-bit flip %zu, a revealed-bit flip %zu, a mask bit beyond the length %zu%s\n", name, p, bad,
               ibad, flip_mask, flip_rev, beyond, len % 8 ? "" : " (8 divides the length: no such bit)");
        bad_total += (int)(bad + ibad) + (flip_mask < 1) + (flip_rev < 1) + (beyond < 1);
    }
}

int main() {
    for (int i = 0; i < 256; i++) sb[i] = aes_sbox_value((uint8_t)i);
    int bad_total = 0;
    run<4>(TRS_HEAD, 1, 1, 13, bad_total);
    run<4>(TRS_MID, 1, 1, 0, bad_total);
    run<4>(TRS_TAIL, 1, 7, 0, bad_total);
    run<4>(TRS_HEAD, 2, 2, 0, bad_total);
    run<4>(TRS_TAIL, 2, 17, 0, bad_total);
    run<8>(TRS_MID, 1, 1, 0, bad_total);
    printf("total bad %d\n", bad_total);
    return bad_total != 0;
}
