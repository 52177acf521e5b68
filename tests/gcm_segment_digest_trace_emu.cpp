// tests/gcm_segment_digest_trace_emu.cpp -- the traces of a DIGEST record's segment keys: k_aes_trace_gcm_seg and k_ghash_trace_seg of
// csrc/kernels_witness.cuh, k_commit_trace and the new k_sha256_trace_seg of csrc/kernels_digest.cuh, and k_witness_expand, run lane by lane ON THE HOST:
// tests/test_gcm_segments_digest_host.py builds this file, which includes the two kernel headers behind tests/lane_emu.h, with -fsanitize=address,undefined.
// Shapes: head c = 4, A = 13; mid c = 4; last Lr = 1, 55, 56, 64; the closing tail (role tail, 0 bytes); an AES-256 mid c = 4.  Every shape is a proof of a real
// digest record -- a head is proof 0 of a record of two data segments, a mid proof 1 of three, a last proof 1 of two, the closing tail proof 2 of two -- so that
// everything the instance is compared with comes from the host-only entries: zkaes_gcm_encrypt_ks, zkaes_gcm_digest_plan, zkaes_gcm_commit.  Two proofs with different
// keys, messages, ivs, aad, salts, H_in and -- proof 1 is hashed behind a 64-byte prefix -- different total_bits per launch; the message, key and header buffers hold
// exactly the bytes that exist, on the heap, and guard bytes lie behind the traces.  The AES kernel is handed the plain headers (its stride is 80 + A), the commitment
// and digest kernels the digest headers with their stride, as ProvingKeyImpl::launch_trace hands them over for its one proof per launch.
// Checked per shape: the circuit's header (digest kind, compressions, the region at TRD of the plain length, the longer header); with every lane of the four kernels run
// alone over traces prefilled with two different patterns, no byte has two writers, the guard bytes and the alignment bytes ahead of the region have none, every byte
// of the digest region has exactly one writing lane, the digest kernel's, which writes nowhere else, and lanes beyond the grids write nothing; after the launch as the
// library makes it, the bytes ahead of the region equal the plain role's trace (head, mid; a last of 64 bytes against the plain mid) under the same inputs.  Per proof:
// every row of (A z) o (B z) = C z holds; the instance is One, what the host says for the role, then (H_in, H_out, total_bits) as the host computed them; a flipped bit
// of H_in, of H_out and of total_bits each leaves at least one row unsatisfied.  No GPU: what the device adds is the launch.
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
static const char *role_name[4] = {"head", "mid", "tail", "last"};
#define CHECK_RC(call) do { if ((call) != 0) { printf("%s: %s\n", #call, zkaes_last_error()); exit(1); } } while (0)

struct Launch {
    int role, kind; uint32_t nproofs, nb, na, len, alen, nblk; size_t kb, stride, seg_off, yout_off, dg_off, hs, plain_hs;
    const uint8_t *msgs, *keys, *hdrs, *plain_hdrs;
    uint32_t lanes(int kernel) const {
        return kernel == 0 ? nproofs * (uint32_t)(TRS_SLOTS(role, nb) + 1) : kernel == 1 ? nproofs * (uint32_t)(TRS_MULS(role, na, nb) + 1) * 16 :
               kernel == 2 ? nproofs * ((role == TRS_MID || role == TRS_LAST) ? 2u : 1u) : nproofs * nblk;
    }
};
enum { K_AES, K_GHASH, K_COMMIT, K_SHA };
template <int NK> static void lane(const Launch &l, int kernel, uint8_t *trace, uint32_t t) {
    blockIdx.x = t;
    if (kernel == K_AES) k_aes_trace_gcm_seg<NK>(trace, l.stride, l.msgs, l.keys, l.plain_hdrs, l.nproofs, (uint32_t)l.role, l.nb, l.na, l.len, l.alen, sb);
    else if (kernel == K_GHASH) k_ghash_trace_seg<NK>(trace, l.stride, l.nproofs, (uint32_t)l.role, l.nb, l.na);
    else if (kernel == K_COMMIT) k_commit_trace(trace, l.stride, l.seg_off, l.yout_off, l.keys, (uint32_t)l.kb, l.hdrs, l.hs, l.nproofs, (uint32_t)l.role, l.nb);
    else k_sha256_trace_seg(trace, l.stride, l.dg_off, l.msgs, l.hdrs, l.hs, l.alen, l.nproofs, l.nblk, l.len, (uint32_t)l.kind);
}
template <int NK> static void launch_all(const Launch &l, uint8_t *trace) {
    for (int k = K_AES; k <= (l.kind ? K_SHA : K_COMMIT); k++) for (uint32_t t = 0; t < l.lanes(k) + 3; t++) lane<NK>(l, k, trace, t);
}
static void put32(uint8_t *p, uint32_t v) { for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (24 - 8 * i)); }

// role: the shape's; c: data blocks per data segment; units: c (head, mid), Lr (last) or 0 (the closing tail); A: the record's aad
template <int NK>
static void run(int role, size_t c, size_t units, size_t A, int &bad_total) {
    const bool closing = role == TRS_TAIL;
    const size_t kb = 4 * NK, len = role == TRS_LAST ? units : closing ? 0 : 16 * c, nb = (len + 15) / 16, seg_a = role == TRS_HEAD ? A : 0, na = (seg_a + 15) / 16;
    // the record around the proof: nd data segments, the proof is number s of nd + 1
    const size_t nd = role == TRS_MID ? 3 : 2, s = role == TRS_HEAD ? 0 : closing ? 2 : 1;
    const size_t L = role == TRS_HEAD ? 16 * c + 9 : role == TRS_MID ? 32 * c + 5 : role == TRS_LAST ? 16 * c + units : 16 * c + 7;
    const int kind = TRS_DG_KIND(role);
    const Circuit cc = compile_aes_gcm_segment_circuit(role, units, seg_a, 8 * kb, 0, 0, 1);
    char name[96];
    snprintf(name, sizeof name, "NK=%d %s c=%zu units=%zu A=%zu", NK, role_name[role], c, units, A);
    const size_t gcm = TRS_GCM(NK, role, nb), sg = gcm + TRS_SEG(role, na, nb), n_mul = TRS_MULS(role, na, nb), ncom = (role == TRS_MID || role == TRS_LAST) ? 2 : 1;
    const size_t plain_bytes = TRS_BYTES(NK, role, na, nb), dg = kind ? TRS_DG(NK, role, na, nb) : 0, nblk = TRD_BLOCKS(kind, len);
    const size_t plain_instance = 1 + 128 + 8 * seg_a + 8 * len + (closing ? 256 : 0) + 256 * ncom;
    if (cc.kind != CIRCUIT_AES_GCM_SEG || cc.seg_role != role || !cc.seg_digest || cc.seg_off != sg || cc.trace_bytes != TRS_DG_BYTES(NK, role, na, nb, kind, len) || cc.trace_bytes % 16 ||
        cc.message_bytes != len || cc.aad_bytes != seg_a || cc.n_blocks != nb || cc.key_bytes != kb || cc.digest_kind != kind || cc.digest_blocks != nblk || cc.digest_off != dg ||
        (kind && (dg % 16 || dg < plain_bytes || dg - plain_bytes >= 16)) || cc.raw_instance != plain_instance + (kind ? 512 : 0) + (kind == 2 ? 64 : 0) ||
        mode_header_bytes(cc) != TRS_HDR_BYTES(seg_a) || segment_header_bytes(cc) != TRS_HDR_DG_BYTES(seg_a, kind) || cc.reveal || cc.key_tag_blocks) {
        printf("%s: circuit header is off\n", name); bad_total++;
    }
    const uint32_t nproofs = 2;
    const size_t plain_hs = TRS_HDR_BYTES(seg_a), hs = TRS_HDR_DG_BYTES(seg_a, kind), stride = cc.trace_bytes, total = stride * nproofs + 64;
    std::unique_ptr<uint8_t[]> msgs(new uint8_t[len * nproofs + 1]), keys(new uint8_t[kb * nproofs]), hdrs(new uint8_t[hs * nproofs]), plain_hdrs(new uint8_t[plain_hs * nproofs]);
    std::vector<std::vector<uint8_t>> rec_ct(nproofs), coms(nproofs), aads(nproofs), ivs(nproofs), states(nproofs);
    std::vector<std::array<uint8_t, 16>> tags(nproofs), lenblks(nproofs);
    std::vector<std::array<uint8_t, 8>> bits(nproofs);
    srand(9300 + 100 * NK + 10 * (unsigned)role + (unsigned)units + (unsigned)A);
    for (uint32_t p = 0; p < nproofs; p++) {
        std::unique_ptr<uint8_t[]> rec(new uint8_t[L]), aad(new uint8_t[A ? A : 1]);
        uint8_t iv[12], salts[48], prefix[64], h0[32];
        for (size_t i = 0; i < L; i++) rec[i] = (uint8_t)rand();
        for (size_t i = 0; i < A; i++) aad[i] = (uint8_t)rand();
        for (auto &x : iv) x = (uint8_t)rand();
        for (auto &x : salts) x = (uint8_t)rand();
        for (auto &x : prefix) x = (uint8_t)rand();
        uint8_t *key = keys.get() + kb * p;
        for (size_t i = 0; i < kb; i++) key[i] = (uint8_t)rand();
        // proof 1's record is hashed behind a 64-byte prefix: another H_in and another total_bits in the same launch
        const uint64_t P = p ? 64 : 0;
        if (p) CHECK_RC(zkaes_sha256_chain(nullptr, prefix, 64, h0));
        rec_ct[p].resize(L); coms[p].resize(32 * nd); aads[p].assign(aad.get(), aad.get() + A); ivs[p].assign(iv, iv + 12); states[p].resize(32 * (nd + 1));
        CHECK_RC(zkaes_gcm_encrypt_ks(rec.get(), L, key, kb, iv, A ? aad.get() : nullptr, A, rec_ct[p].data(), tags[p].data()));
        std::unique_ptr<uint8_t[]> ys(new uint8_t[16 * nd]);
        size_t n_data = 0;
        CHECK_RC(zkaes_gcm_digest_plan(rec.get(), L, key, kb, iv, A ? aad.get() : nullptr, A, c, p ? h0 : nullptr, P, ys.get(), 16 * nd, states[p].data(), 32 * (nd + 1), &n_data));
        if (n_data != nd) { printf("%s: the record has %zu data segments, not %zu\n", name, n_data, nd); bad_total++; }
        for (size_t b = 0; b < nd; b++) CHECK_RC(zkaes_gcm_commit(key, kb, ys.get() + 16 * b, salts + 16 * b, coms[p].data() + 32 * b));
        const uint64_t total_bits = 8 * (P + (uint64_t)L);
        for (int i = 0; i < 8; i++) { lenblks[p][i] = (uint8_t)((uint64_t)(8 * A) >> (56 - 8 * i)); lenblks[p][8 + i] = (uint8_t)((uint64_t)(8 * L) >> (56 - 8 * i)); bits[p][i] = (uint8_t)(total_bits >> (56 - 8 * i)); }
        if (len) memcpy(msgs.get() + len * p, rec.get() + 16 * c * s, len);
        uint8_t *h = hdrs.get() + hs * p;
        memset(h, 0, hs);
        memcpy(h + TRS_HDR_IV, iv, 12);
        put32(h + TRS_HDR_CTR0, (uint32_t)(2 + s * c));
        if (s) { memcpy(h + TRS_HDR_YIN, ys.get() + 16 * (s - 1), 16); memcpy(h + TRS_HDR_SALT_IN, salts + 16 * (s - 1), 16); }
        if (s < nd) memcpy(h + TRS_HDR_SALT_OUT, salts + 16 * s, 16);
        memcpy(h + TRS_HDR_LEN, lenblks[p].data(), 16);
        if (seg_a) memcpy(h + TRS_HDR_AAD, aad.get(), seg_a);
        memcpy(plain_hdrs.get() + plain_hs * p, h, plain_hs);
        if (kind) memcpy(h + TRS_HDR_HIN(seg_a), states[p].data() + 32 * s, 32);
        if (kind == 2) memcpy(h + TRS_HDR_BITS(seg_a), bits[p].data(), 8);
    }
    const size_t yout_off = gcm + TR_GCM_MUL0(na, nb) + (n_mul - 1) * TR_GCM_MUL_STRIDE + TR_GCM_MUL_Y;
    Launch l{role, kind, nproofs, (uint32_t)nb, (uint32_t)na, (uint32_t)len, (uint32_t)seg_a, (uint32_t)nblk, kb, stride, sg, yout_off, dg, hs, plain_hs, msgs.get(), keys.get(), hdrs.get(), plain_hdrs.get()};
    // ---- who writes what: every lane of every kernel alone, over two prefill patterns (a byte is written iff it leaves either pattern; Y_out, which a com_out lane reads,
    // holds random bytes in both, as in tests/gcm_segment_trace_emu.cpp)
    std::vector<uint32_t> writers(total, 0), sha_writers(total, 0);
    size_t lane_bad = 0;
    std::vector<uint8_t> fill_a(total, 0xAA), fill_b(total, 0x55);
    for (uint32_t p = 0; p < nproofs; p++) for (int i = 0; i < 16; i++) { fill_a[p * stride + yout_off + i] = (uint8_t)rand(); fill_b[p * stride + yout_off + i] = (uint8_t)rand(); }
    auto alone = [&](int kernel, uint32_t t, uint32_t lanes) {
        std::vector<uint8_t> a(fill_a), b(fill_b);
        for (std::vector<uint8_t> *tr : {&a, &b}) lane<NK>(l, kernel, tr->data(), t);
        size_t wrote = 0;
        for (size_t i = 0; i < total; i++) if (a[i] != fill_a[i] || b[i] != fill_b[i]) { writers[i]++; wrote++; if (kernel == K_SHA) sha_writers[i]++; }
        if (t >= lanes && wrote) { printf("%s: a lane of kernel %d beyond the grid wrote to the trace\n", name, kernel); lane_bad++; }
    };
    for (int k = K_AES; k <= (kind ? K_SHA : K_COMMIT); k++) for (uint32_t t = 0; t < l.lanes(k) + 3; t++) alone(k, t, l.lanes(k));
    size_t two_writers = 0, guard_writers = 0, region_bad = 0, sha_elsewhere = 0, padding_written = 0;
    for (size_t i = 0; i < total; i++) {
        if (i >= stride * nproofs) { guard_writers += writers[i] != 0; continue; }
        two_writers += writers[i] > 1;
        const size_t o = i % stride;
        if (kind && o >= dg) region_bad += writers[i] != 1 || sha_writers[i] != 1;                      // one writing lane per byte of the region, the digest kernel's
        else sha_elsewhere += sha_writers[i] != 0;                                                      // and none elsewhere from it
        if (kind && o >= plain_bytes && o < dg) padding_written += writers[i] != 0;
    }
    printf("%s: bytes with two writers %zu, guard bytes written %zu, alignment bytes written %zu, digest region bytes without their one digest lane %zu, bytes elsewhere the digest kernel wrote %zu, "
           "lane faults %zu\n", name, two_writers, guard_writers, padding_written, region_bad, sha_elsewhere, lane_bad);
    bad_total += (two_writers != 0) + (guard_writers != 0) + (padding_written != 0) + (region_bad != 0) + (sha_elsewhere != 0) + (lane_bad != 0);
    // ---- the launch as the library makes it
    std::vector<uint8_t> trace(total, 0xAA);
    launch_all<NK>(l, trace.data());
    for (size_t i = stride * nproofs; i < total; i++) if (trace[i] != 0xAA) { printf("%s: write past the traces\n", name); bad_total++; break; }
    // the bytes ahead of the region are the plain role's trace: a head or mid against its own role without the flag, a last of 16 c bytes against the plain mid of c
    if (role == TRS_HEAD || role == TRS_MID || (role == TRS_LAST && len == 16 * c)) {
        const int plain_role = role == TRS_LAST ? TRS_MID : role;
        const Circuit plain = compile_aes_gcm_segment_circuit(plain_role, c, seg_a, 8 * kb);
        Launch lp = l;
        lp.role = plain_role; lp.kind = 0; lp.stride = plain.trace_bytes; lp.hdrs = plain_hdrs.get(); lp.hs = plain_hs;
        std::vector<uint8_t> plain_trace(plain.trace_bytes * nproofs + 64, 0xAA);
        launch_all<NK>(lp, plain_trace.data());
        size_t differs = plain.trace_bytes != plain_bytes;
        for (uint32_t p = 0; p < nproofs; p++) differs += memcmp(trace.data() + p * stride, plain_trace.data() + p * plain.trace_bytes, plain_bytes) != 0;
        printf("%s: proofs whose bytes ahead of the digest region differ from the plain %s trace %zu\n", name, role_name[plain_role], differs);
        bad_total += differs != 0;
    }
    for (uint32_t p = 0; p < nproofs; p++) {
        const uint8_t *tr = trace.data() + p * stride;
        std::vector<uint8_t> z(cc.num_variables());
        for (uint32_t i = 0; i < z.size(); i++) { blockIdx.x = i; k_witness_expand(z.data(), cc.desc.data(), (uint32_t)z.size(), tr, cc.sbox_in_off.data(), cc.sbox_tmpl.data(), sb); }
        const size_t bad = unsatisfied(cc, z);
        // the instance: One, iv, ctr0, (aad), the ciphertext slice, (length block, tag), (com_in), (com_out), then H_in, H_out, (total_bits), zero padding
        size_t ibad = z[0] != 1, at = 1;
        auto expect = [&](const uint8_t *d, size_t nbytes) { for (size_t i = 0; i < nbytes; i++) for (int k = 0; k < 8; k++) ibad += z[at++] != ((d[i] >> k) & 1); };
        uint8_t ctr0[4];
        put32(ctr0, (uint32_t)(2 + s * c));
        expect(ivs[p].data(), 12);
        expect(ctr0, 4);
        if (seg_a) expect(aads[p].data(), seg_a);
        if (len) expect(rec_ct[p].data() + 16 * c * s, len);
        if (closing) { expect(lenblks[p].data(), 16); expect(tags[p].data(), 16); }
        if (role != TRS_HEAD) expect(coms[p].data() + 32 * (s - 1), 32);
        if (!closing) expect(coms[p].data() + 32 * s, 32);
        if (at != plain_instance) ibad++;
        const size_t hin_at = at;
        if (kind) expect(states[p].data() + 32 * s, 64);
        const size_t bits_at = at;
        if (kind == 2) expect(bits[p].data(), 8);
        if (at != cc.raw_instance) ibad++;
        for (; at < cc.num_instance; at++) ibad += z[at] != 0;
        if (kind == 2 && memcmp(states[p].data() + 32 * nd, tr + dg + TRD_HOUT, 32) != 0) ibad++;      // the trace's H_out is the record's real digest
        auto flipped = [&](size_t where) { std::vector<uint8_t> zf(z); zf[where] ^= 1; return unsatisfied(cc, zf); };
        const size_t flip_hin = kind ? flipped(hin_at + 8 * (5 + 7 * p) + 3) : 1, flip_hout = kind ? flipped(hin_at + 256 + 8 * (9 + 11 * p) + 6) : 1, flip_bits = kind == 2 ? flipped(bits_at + 8 * 7 + 3 + p) : 1;
        const size_t flip_tag = closing ? flipped(1 + 128 + 128 + 8 * (2 + p) + 1) : 1;
        printf("%s proof %u: unsatisfied %zu, instance mismatches %zu, rows unsatisfied after a flip of H_in %zu, H_out %zu, total_bits %zu, the tag %zu\n", name, p, bad, ibad, flip_hin, flip_hout,
               flip_bits, flip_tag);
        bad_total += (int)(bad + ibad) + (flip_hin < 1) + (flip_hout < 1) + (flip_bits < 1) + (flip_tag < 1);
    }
}

int main() {
    for (int i = 0; i < 256; i++) sb[i] = aes_sbox_value((uint8_t)i);
    int bad_total = 0;
    run<4>(TRS_HEAD, 4, 4, 13, bad_total);
    run<4>(TRS_MID, 4, 4, 0, bad_total);
    run<4>(TRS_LAST, 4, 1, 3, bad_total);
    run<4>(TRS_LAST, 4, 55, 0, bad_total);
    run<4>(TRS_LAST, 4, 56, 0, bad_total);
    run<4>(TRS_LAST, 4, 64, 5, bad_total);
    run<4>(TRS_TAIL, 4, 0, 13, bad_total);
    run<8>(TRS_MID, 4, 4, 0, bad_total);
    printf("total bad %d\n", bad_total);
    return bad_total != 0;
}
