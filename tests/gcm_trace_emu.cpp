// tests/gcm_trace_emu.cpp -- k_aes_trace_gcm, k_ghash_trace and k_witness_expand of csrc/kernels_witness.cuh run lane by lane ON THE HOST: tests/test_gcm_host.py builds
// this file, which includes that header behind tests/lane_emu.h, with -fsanitize=address,undefined.  Shapes: (L, A) = (1, 0), (16, 0),
// (17, 5), (16, 20), (33, 16), two proofs per launch.  The message buffer holds exactly nproofs * L bytes and the header buffer exactly nproofs * (12 + A) bytes on the
// heap, so a lane that reads past a partial block is a sanitizer report; guard bytes lie behind the traces, and every byte of the GCM tail must have been written.
// Checked per proof: every row of (A z) o (B z) = C z holds; the instance is One, the iv, aad, ciphertext and tag bits of zkaes_gcm_encrypt, zero padding; every q byte
// is at most 64; flipping one tag bit of the instance leaves exactly one row unsatisfied, flipping one aad bit (where there is aad) or one iv bit at least one.  No GPU:
// what the device adds is the launch.
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
int main() {
    uint8_t sb[256]; for (int i = 0; i < 256; i++) sb[i] = aes_sbox_value((uint8_t)i);
    int bad_total = 0;
    const size_t shapes[5][2] = {{1, 0}, {16, 0}, {17, 5}, {16, 20}, {33, 16}};
    for (int shape = 0; shape < 5; shape++) {
        const size_t L = shapes[shape][0], A = shapes[shape][1], nb = (L + 15) / 16, na = (A + 15) / 16, n_mul = na + nb + 1, hs = 12 + A;
        Circuit c = compile_aes_gcm_circuit(L, A);
        if (c.trace_bytes != TR_GCM_BYTES(na, nb) || c.trace_bytes % 16 || c.message_bytes != L || c.aad_bytes != A || c.n_blocks != nb || c.raw_instance != 225 + 8 * (A + L)) {
            printf("L=%zu A=%zu: circuit header is off\n", L, A); bad_total++;
        }
        const uint32_t nproofs = 2;
        std::unique_ptr<uint8_t[]> msgs(new uint8_t[L * nproofs]), hdrs(new uint8_t[hs * nproofs]);          // exactly the bytes that exist
        std::vector<uint8_t> keys(16 * nproofs), trace(c.trace_bytes * nproofs + 64, 0xAA);
        srand(200 + shape);
        for (size_t i = 0; i < L * nproofs; i++) msgs[i] = (uint8_t)rand();
        for (size_t i = 0; i < hs * nproofs; i++) hdrs[i] = (uint8_t)rand();
        for (auto &x : keys) x = (uint8_t)rand();
        if (shape == 1) { memset(keys.data() + 16, 0, 16); memset(msgs.get() + L, 0, L); memset(hdrs.get() + hs, 0, hs); }          // McGrew-Viega test case 2 as the second proof
        // the tail is written by these two kernels alone: poison it so that a byte nobody wrote shows
        for (uint32_t p = 0; p < nproofs; p++) memset(trace.data() + p * c.trace_bytes + TR_GCM(nb), 0x5C, c.trace_bytes - TR_GCM(nb));
        for (uint32_t t = 0; t < nproofs * (nb + 3) + 3; t++) {
            blockIdx.x = t;
            k_aes_trace_gcm(trace.data(), c.trace_bytes, msgs.get(), keys.data(), hdrs.get(), nproofs, (uint32_t)nb, (uint32_t)na, (uint32_t)L, (uint32_t)A, sb);
        }
        for (uint32_t t = 0; t < nproofs * (n_mul + 1) * 16 + 3; t++) {
            blockIdx.x = t;
            k_ghash_trace(trace.data(), c.trace_bytes, nproofs, (uint32_t)nb, (uint32_t)na, (uint32_t)L, (uint32_t)A);
        }
        for (size_t i = c.trace_bytes * nproofs; i < trace.size(); i++) if (trace[i] != 0xAA) { printf("write past the traces\n"); bad_total++; }
        for (uint32_t p = 0; p < nproofs; p++) {
            const uint8_t *tr = trace.data() + p * c.trace_bytes, *tail = tr + TR_GCM(nb);
            std::vector<uint8_t> z(c.num_variables());
            for (uint32_t i = 0; i < z.size(); i++) { blockIdx.x = i; k_witness_expand(z.data(), c.desc.data(), (uint32_t)z.size(), tr, c.sbox_in_off.data(), c.sbox_tmpl.data(), sb); }
            size_t bad = unsatisfied(c, z);
            std::unique_ptr<uint8_t[]> ct(new uint8_t[L]);
            uint8_t tag[16];
            const uint8_t *hdr = hdrs.get() + hs * p;
            if (zkaes_gcm_encrypt(msgs.get() + L * p, L, keys.data() + 16 * p, hdr, A ? hdr + 12 : nullptr, A, ct.get(), tag) != 0) { printf("zkaes_gcm_encrypt: %s\n", zkaes_last_error()); return 1; }
            size_t ibad = z[0] != 1, at = 1;
            for (size_t i = 0; i < hs; i++) for (int k = 0; k < 8; k++) ibad += z[at++] != ((hdr[i] >> k) & 1);
            for (size_t i = 0; i < L; i++) for (int k = 0; k < 8; k++) ibad += z[at++] != ((ct[i] >> k) & 1);
            const size_t tag_at = at;
            for (size_t i = 0; i < 16; i++) for (int k = 0; k < 8; k++) ibad += z[at++] != ((tag[i] >> k) & 1);
            if (at != c.raw_instance) ibad++;
            for (; at < c.num_instance; at++) ibad += z[at] != 0;
            // the tail: zeros beyond the aad and the ciphertext, every q byte <= 64, the padding of the iv slot, the second proof of shape 1 is test case 2
            size_t tbad = 0;
            for (size_t i = A; i < 16 * na; i++) tbad += tail[TR_GCM_AAD + i] != 0;
            for (size_t i = L; i < 16 * nb; i++) tbad += tail[TR_GCM_CT(na) + i] != 0 || tr[TR_BLOCK0 + (i / 16) * TR_BLOCK_STRIDE + TR_BL_MSG + i % 16] != 0;
            for (size_t i = 12; i < 16; i++) tbad += tail[TR_GCM_IV + i] != 0;
            for (size_t m = 0; m < n_mul; m++) for (int k = 0; k < 128; k++) tbad += tail[TR_GCM_MUL0(na, nb) + m * TR_GCM_MUL_STRIDE + TR_GCM_MUL_Q + k] > 64;
            tbad += memcmp(tail + TR_GCM_TAG(na, nb), tag, 16) != 0;
            if (shape == 1 && p == 1) {
                const uint8_t want[16] = {0xab, 0x6e, 0x47, 0xd4, 0x2c, 0xec, 0x13, 0xbd, 0xf5, 0x3a, 0x67, 0xb2, 0x12, 0x57, 0xbd, 0xdf};
                tbad += memcmp(tail + TR_GCM_TAG(na, nb), want, 16) != 0;
            }
            std::vector<uint8_t> zf(z);
            zf[tag_at + 8 * 5 + 3] ^= 1;                                      // a tag bit
            size_t flip_tag = unsatisfied(c, zf);
            size_t flip_aad = 1;
            if (A) { zf = z; zf[1 + 96 + 8 * (A - 1) + 6] ^= 1; flip_aad = unsatisfied(c, zf); }       // a bit of the last aad byte (in the partial block where there is one)
            zf = z; zf[1 + 8 * 11] ^= 1;                                      // bit 0 of the last iv byte
            size_t flip_iv = unsatisfied(c, zf);
            printf("L=%zu A=%zu proof %u: unsatisfied %zu, instance mismatches %zu, tail mismatches %zu, rows unsatisfied after a tag flip %zu, after an aad flip %zu, after an iv flip %zu\n",
                   L, A, p, bad, ibad, tbad, flip_tag, flip_aad, flip_iv);
            bad_total += (int)(bad + ibad + tbad) + (flip_tag != 1) + (flip_aad < 1) + (flip_iv < 1);
        }
        // every byte of the tail has a writer
        for (uint32_t p = 0; p < nproofs; p++) {
            // (a written byte may equal the poison by chance; what cannot is a run of them: the unwritten regions would be whole 16-byte slots)
            const uint8_t *tail = trace.data() + p * c.trace_bytes + TR_GCM(nb);
            size_t run = 0, worst = 0;
            for (size_t i = 0; i < c.trace_bytes - TR_GCM(nb); i++) { run = tail[i] == 0x5C ? run + 1 : 0; if (run > worst) worst = run; }
            if (worst >= 8) { printf("L=%zu A=%zu proof %u: %zu bytes of the tail in a row were never written\n", L, A, p, worst); bad_total++; }
        }
    }
    printf("total bad %d\n", bad_total);
    return bad_total != 0;
}
