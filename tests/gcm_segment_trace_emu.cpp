// tests/gcm_segment_trace_emu.cpp -- k_aes_trace_gcm_seg and k_ghash_trace_seg of csrc/kernels_witness.cuh, k_commit_trace of csrc/kernels_digest.cuh and
// k_witness_expand, run lane by lane ON THE HOST: tests/test_gcm_segments_host.py builds this file, which includes the two kernel headers behind
// tests/lane_emu.h, with -fsanitize=address,undefined.  Shapes: head (A = 5, c = 1), head (A = 0, c = 2), mid (c = 1), mid (c = 2), tail (Lt = 7, c = 1), tail
// (Lt = 32, c = 2), an AES-256 mid (c = 1).  Every shape is a segment of a real record -- a head is segment 0 of a two-segment record, a mid segment 1 of three, a tail
// segment 1 of two -- so that everything the instance is compared with comes from the host-only entries: zkaes_gcm_encrypt_ks, zkaes_gcm_boundaries, zkaes_gcm_commit.
// Two proofs with different keys, messages, ivs, aad and salts per launch; the message, key and header buffers hold exactly the bytes that exist, on the heap, and guard
// bytes lie behind the traces.
// Checked per shape: the circuit's header; with every lane of the three kernels run alone over traces prefilled with two different patterns, no byte of the traces has
// two writers, the guard bytes have none, every byte of the segment region that the role uses has one, a commitment lane writes its 32 + 4032 bytes and nothing ahead of
// the region, lanes beyond the grids write nothing.  Per proof: every row of (A z) o (B z) = C z holds; the instance is One, then what the host says; a flipped bit of
// com_in, com_out, ctr0 and the length block (where the role has them) each leaves at least one row unsatisfied.  Last, a mid (c = 2) whose ctr0 is 2^32 - 1: the counter
// wraps mod 2^32 and leaves the iv alone, every row holds, and the ciphertext is the keystream of iv || ffffffff, iv || 00000000.  No GPU: what the device adds is the launch.
#include "circuit.hpp"
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
    int role; uint32_t nproofs, nb, na, len, alen; size_t kb, stride, seg_off, yout_off, hs;
    const uint8_t *msgs, *keys, *hdrs;
    uint32_t aes_lanes() const { return nproofs * (uint32_t)(TRS_SLOTS(role, nb) + 1); }
    uint32_t ghash_lanes() const { return nproofs * (uint32_t)(TRS_MULS(role, na, nb) + 1) * 16; }
    uint32_t commit_lanes() const { return nproofs * (role == TRS_MID ? 2u : 1u); }
};
template <int NK> static void aes_lane(const Launch &l, uint8_t *trace, uint32_t t) { blockIdx.x = t; k_aes_trace_gcm_seg<NK>(trace, l.stride, l.msgs, l.keys, l.hdrs, l.nproofs, (uint32_t)l.role, l.nb, l.na, l.len, l.alen, sb); }
template <int NK> static void ghash_lane(const Launch &l, uint8_t *trace, uint32_t t) { blockIdx.x = t; k_ghash_trace_seg<NK>(trace, l.stride, l.nproofs, (uint32_t)l.role, l.nb, l.na); }
static void commit_lane(const Launch &l, uint8_t *trace, uint32_t t) { blockIdx.x = t; k_commit_trace(trace, l.stride, l.seg_off, l.yout_off, l.keys, (uint32_t)l.kb, l.hdrs, l.hs, l.nproofs, (uint32_t)l.role, l.nb); }
template <int NK> static void launch_all(const Launch &l, uint8_t *trace) {
    for (uint32_t t = 0; t < l.aes_lanes() + 3; t++) aes_lane<NK>(l, trace, t);
    for (uint32_t t = 0; t < l.ghash_lanes() + 3; t++) ghash_lane<NK>(l, trace, t);
    for (uint32_t t = 0; t < l.commit_lanes() + 3; t++) commit_lane(l, trace, t);
}
static void put32(uint8_t *p, uint32_t v) { for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (24 - 8 * i)); }

// role: the shape's; c: data blocks per segment; units: c (head, mid) or Lt (tail); A: the record's aad
template <int NK>
static void run(int role, size_t c, size_t units, size_t A, int &bad_total) {
    const size_t kb = 4 * NK, len = role == TRS_TAIL ? units : 16 * c, nb = (len + 15) / 16, seg_a = role == TRS_HEAD ? A : 0, na = (seg_a + 15) / 16;
    const size_t s = role == TRS_HEAD ? 0 : 1, n = role == TRS_MID ? 3 : 2, L = role == TRS_HEAD ? 16 * c + 9 : role == TRS_MID ? 32 * c + 5 : 16 * c + units;      // the record around the segment
    const Circuit cc = compile_aes_gcm_segment_circuit(role, units, seg_a, 8 * kb);
    char name[96];
    snprintf(name, sizeof name, "NK=%d %s c=%zu units=%zu A=%zu", NK, role_name[role], c, units, A);
    const size_t gcm = TRS_GCM(NK, role, nb), sg = gcm + TRS_SEG(role, na, nb), n_mul = TRS_MULS(role, na, nb), ncom = role == TRS_MID ? 2 : 1;
    if (cc.kind != CIRCUIT_AES_GCM_SEG || cc.seg_role != role || cc.seg_off != sg || cc.trace_bytes != TRS_BYTES(NK, role, na, nb) || cc.trace_bytes % 16 || cc.message_bytes != len || cc.aad_bytes != seg_a ||
        cc.n_blocks != nb || cc.key_bytes != kb || cc.raw_instance != 1 + 128 + 8 * seg_a + 8 * len + (role == TRS_TAIL ? 256 : 0) + 256 * ncom || mode_header_bytes(cc) != TRS_HDR_BYTES(seg_a)) {
        printf("%s: circuit header is off\n", name); bad_total++;
    }
    const uint32_t nproofs = 2;
    const size_t hs = TRS_HDR_BYTES(seg_a), stride = cc.trace_bytes, total = stride * nproofs + 64;
    std::unique_ptr<uint8_t[]> msgs(new uint8_t[len * nproofs]), keys(new uint8_t[kb * nproofs]), hdrs(new uint8_t[hs * nproofs]);      // exactly the bytes that exist
    std::vector<std::vector<uint8_t>> rec_ct(nproofs), coms(nproofs), aads(nproofs), ivs(nproofs);
    std::vector<std::array<uint8_t, 16>> tags(nproofs), lenblks(nproofs);
    srand(7100 + 100 * NK + 10 * (unsigned)role + (unsigned)units + (unsigned)A);
    for (uint32_t p = 0; p < nproofs; p++) {
        std::unique_ptr<uint8_t[]> rec(new uint8_t[L]), aad(new uint8_t[A ? A : 1]);
        uint8_t iv[12], salts[32];
        for (size_t i = 0; i < L; i++) rec[i] = (uint8_t)rand();
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
        memcpy(msgs.get() + len * p, rec.get() + 16 * c * s, len);
        uint8_t *h = hdrs.get() + hs * p;
        memset(h, 0, hs);
        memcpy(h + TRS_HDR_IV, iv, 12);
        put32(h + TRS_HDR_CTR0, (uint32_t)(2 + s * c));
        if (s) { memcpy(h + TRS_HDR_YIN, ys.get() + 16 * (s - 1), 16); memcpy(h + TRS_HDR_SALT_IN, salts + 16 * (s - 1), 16); }
        if (s + 1 < n) memcpy(h + TRS_HDR_SALT_OUT, salts + 16 * s, 16);
        memcpy(h + TRS_HDR_LEN, lenblks[p].data(), 16);
        if (seg_a) memcpy(h + TRS_HDR_AAD, aad.get(), seg_a);
    }
    Launch l{role, nproofs, (uint32_t)nb, (uint32_t)na, (uint32_t)len, (uint32_t)seg_a, kb, stride, sg, gcm + TR_GCM_MUL0(na, nb) + (n_mul - 1) * TR_GCM_MUL_STRIDE + TR_GCM_MUL_Y, hs, msgs.get(), keys.get(), hdrs.get()};
    // ---- who writes what: every lane of the three kernels alone, over two prefill patterns (a byte is written iff it leaves either pattern)
    std::vector<uint32_t> writers(total, 0);
    size_t lane_bad = 0;
    // (a com_out lane READS Y_out from the trace: were it a run of the pattern's byte, the compression's shifted words would repeat that byte and pass for unwritten, so
    // the two prefills hold random bytes there)
    std::vector<uint8_t> fill_a(total, 0xAA), fill_b(total, 0x55);
    for (uint32_t p = 0; p < nproofs; p++) for (int i = 0; i < 16; i++) { fill_a[p * stride + l.yout_off + i] = (uint8_t)rand(); fill_b[p * stride + l.yout_off + i] = (uint8_t)rand(); }
    auto alone = [&](int kernel, uint32_t t, uint32_t lanes) {
        std::vector<uint8_t> a(fill_a), b(fill_b);
        for (std::vector<uint8_t> *tr : {&a, &b}) { if (kernel == 0) aes_lane<NK>(l, tr->data(), t); else if (kernel == 1) ghash_lane<NK>(l, tr->data(), t); else commit_lane(l, tr->data(), t); }
        size_t wrote = 0, ahead = 0;
        for (size_t i = 0; i < total; i++) if (a[i] != fill_a[i] || b[i] != fill_b[i]) { writers[i]++; wrote++; ahead += i % stride < sg + TRS_COM_IN; }
        if (t >= lanes && wrote) { printf("%s: a lane of kernel %d beyond the grid wrote to the trace\n", name, kernel); lane_bad++; }
        if (kernel == 2 && t < lanes && (wrote != 32 + 4032 || ahead)) { printf("%s: commitment lane %u wrote %zu bytes, %zu of them ahead of the commitments\n", name, t, wrote, ahead); lane_bad++; }
    };
    for (uint32_t t = 0; t < l.aes_lanes() + 3; t++) alone(0, t, l.aes_lanes());
    for (uint32_t t = 0; t < l.ghash_lanes() + 3; t++) alone(1, t, l.ghash_lanes());
    for (uint32_t t = 0; t < l.commit_lanes() + 3; t++) alone(2, t, l.commit_lanes());
    size_t two_writers = 0, guard_writers = 0, region_unwritten = 0;
    for (size_t i = 0; i < total; i++) {
        if (i >= stride * nproofs) { guard_writers += writers[i] != 0; continue; }
        two_writers += writers[i] > 1;
        const size_t o = i % stride;
        if (o < sg) continue;
        const size_t r = o - sg;                                                                   // the region's bytes this role uses have exactly one writer
        bool used = r < TRS_COM_IN || (r >= TRS_BLOCK_CTR0 && r < TRS_BLOCK_CTR0 + TRS_BLOCK_CTR_STRIDE * nb);
        if (role != TRS_HEAD) used = used || (r >= TRS_COM_IN && r < TRS_COM_OUT) || (r >= TRS_SLOT_IN(nb) && r < TRS_SLOT_OUT(nb));
        if (role != TRS_TAIL) used = used || (r >= TRS_COM_OUT && r < TRS_BLOCK_CTR0) || r >= TRS_SLOT_OUT(nb);
        region_unwritten += used && writers[i] != 1;
        two_writers += !used && writers[i] != 0;                                                   // ... and the others none
    }
    printf("%s: bytes with two writers %zu, guard bytes written %zu, used region bytes without their one writer %zu, lane faults %zu\n", name, two_writers, guard_writers, region_unwritten, lane_bad);
    bad_total += (two_writers != 0) + (guard_writers != 0) + (region_unwritten != 0) + (lane_bad != 0);
    // ---- the launch as the library makes it
    std::vector<uint8_t> trace(total, 0xAA);
    launch_all<NK>(l, trace.data());
    for (size_t i = stride * nproofs; i < total; i++) if (trace[i] != 0xAA) { printf("%s: write past the traces\n", name); bad_total++; break; }
    for (uint32_t p = 0; p < nproofs; p++) {
        const uint8_t *tr = trace.data() + p * stride;
        std::vector<uint8_t> z(cc.num_variables());
        for (uint32_t i = 0; i < z.size(); i++) { blockIdx.x = i; k_witness_expand(z.data(), cc.desc.data(), (uint32_t)z.size(), tr, cc.sbox_in_off.data(), cc.sbox_tmpl.data(), sb); }
        const size_t bad = unsatisfied(cc, z);
        // the instance: One, iv, ctr0, (aad), the ciphertext slice, (length block, tag), (com_in), (com_out), zero padding
        size_t ibad = z[0] != 1, at = 1;
        auto expect = [&](const uint8_t *d, size_t nbytes) { for (size_t i = 0; i < nbytes; i++) for (int k = 0; k < 8; k++) ibad += z[at++] != ((d[i] >> k) & 1); };
        uint8_t ctr0[4];
        put32(ctr0, (uint32_t)(2 + s * c));
        expect(ivs[p].data(), 12);
        const size_t ctr0_at = at;
        expect(ctr0, 4);
        if (seg_a) expect(aads[p].data(), seg_a);
        expect(rec_ct[p].data() + 16 * c * s, len);
        const size_t len_at = at;
        if (role == TRS_TAIL) { expect(lenblks[p].data(), 16); expect(tags[p].data(), 16); }
        const size_t com_in_at = at;
        if (role != TRS_HEAD) expect(coms[p].data() + 32 * (s - 1), 32);
        const size_t com_out_at = at;
        if (role != TRS_TAIL) expect(coms[p].data() + 32 * s, 32);
        if (at != cc.raw_instance) ibad++;
        for (; at < cc.num_instance; at++) ibad += z[at] != 0;
        auto flipped = [&](size_t where) { std::vector<uint8_t> zf(z); zf[where] ^= 1; return unsatisfied(cc, zf); };
        const size_t flip_ctr0 = flipped(ctr0_at + 8 * 3 + 1), flip_len = role == TRS_TAIL ? flipped(len_at + 8 * 15 + 4) : 1;
        const size_t flip_in = role != TRS_HEAD ? flipped(com_in_at + 8 * (3 + 11 * p) + 5) : 1, flip_out = role != TRS_TAIL ? flipped(com_out_at + 8 * (7 + 9 * p) + 2) : 1;
        printf("%s proof %u: unsatisfied %zu, instance mismatches %zu, rows unsatisfied after a flip of ctr0 %zu, the length block %zu, com_in %zu, com_out %zu\n", name, p, bad, ibad, flip_ctr0,
               flip_len, flip_in, flip_out);
        bad_total += (int)(bad + ibad) + (flip_ctr0 < 1) + (flip_len < 1) + (flip_in < 1) + (flip_out < 1);
    }
}

// a mid of two blocks whose first counter is 2^32 - 1: the second block runs under iv || 00000000
static void run_wrap(int &bad_total) {
    const size_t kb = 16, len = 32, hs = TRS_HDR_BYTES(0);
    const Circuit cc = compile_aes_gcm_segment_circuit(TRS_MID, 2, 0, 128);
    std::unique_ptr<uint8_t[]> msg(new uint8_t[len]), key(new uint8_t[kb]), hdr(new uint8_t[hs]);
    srand(7777);
    for (size_t i = 0; i < len; i++) msg[i] = (uint8_t)rand();
    for (size_t i = 0; i < kb; i++) key[i] = (uint8_t)rand();
    for (size_t i = 0; i < hs; i++) hdr[i] = (uint8_t)rand();
    put32(hdr.get() + TRS_HDR_CTR0, 0xffffffffu);
    const size_t gcm = TRS_GCM(4, TRS_MID, 2), sg = gcm + TRS_SEG(TRS_MID, 0, 2);
    Launch l{TRS_MID, 1, 2, 0, (uint32_t)len, 0, kb, cc.trace_bytes, sg, gcm + TR_GCM_MUL0(0, 2) + TR_GCM_MUL_STRIDE + TR_GCM_MUL_Y, hs, msg.get(), key.get(), hdr.get()};
    std::vector<uint8_t> trace(cc.trace_bytes + 64, 0xAA), z(cc.num_variables());
    launch_all<4>(l, trace.data());
    for (uint32_t i = 0; i < z.size(); i++) { blockIdx.x = i; k_witness_expand(z.data(), cc.desc.data(), (uint32_t)z.size(), trace.data(), cc.sbox_in_off.data(), cc.sbox_tmpl.data(), sb); }
    const size_t bad = unsatisfied(cc, z);
    uint8_t blocks[32], stream[32];
    memcpy(blocks, hdr.get(), 12); put32(blocks + 12, 0xffffffffu); memcpy(blocks + 16, hdr.get(), 12); put32(blocks + 28, 0);
    CHECK_RC(zkaes_ecb_ciphertext_ks(blocks, 32, key.get(), kb, stream));
    size_t ibad = 0, at = 1 + 128;
    for (size_t i = 0; i < len; i++) for (int k = 0; k < 8; k++) ibad += z[at++] != (((msg[i] ^ stream[i]) >> k) & 1);
    const uint8_t *cs = trace.data() + sg + TRS_BLOCK_CTR0 + TRS_BLOCK_CTR_STRIDE;
    const uint8_t want[8] = {0, 0, 0, 0, 0x7f, 0xff, 0xff, 0xff};                                  // the counter of block 1, and carries out of positions 0 .. 30
    ibad += memcmp(cs, want, 8) != 0;
    printf("wrap: unsatisfied %zu, mismatches %zu\n", bad, ibad);
    bad_total += (int)(bad + ibad);
}

int main() {
    for (int i = 0; i < 256; i++) sb[i] = aes_sbox_value((uint8_t)i);
    int bad_total = 0;
    run<4>(TRS_HEAD, 1, 1, 5, bad_total);
    run<4>(TRS_HEAD, 2, 2, 0, bad_total);
    run<4>(TRS_MID, 1, 1, 3, bad_total);
    run<4>(TRS_MID, 2, 2, 0, bad_total);
    run<4>(TRS_TAIL, 1, 7, 5, bad_total);
    run<4>(TRS_TAIL, 2, 32, 0, bad_total);
    run<8>(TRS_MID, 1, 1, 20, bad_total);
    run_wrap(bad_total);
    printf("total bad %d\n", bad_total);
    return bad_total != 0;
}
