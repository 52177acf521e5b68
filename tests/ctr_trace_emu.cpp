// tests/ctr_trace_emu.cpp -- k_aes_trace_ctr and k_witness_expand of csrc/kernels_witness.cuh run lane by lane ON THE HOST: tests/test_ctr_host.py builds this file,
// which includes that header behind tests/lane_emu.h, with -fsanitize=address,undefined.  Shapes: L = 1, 16, 17, 33, 48 bytes, two proofs per
// launch under different counters, the counters whose increment carries furthest among them (ff..ff wraps to zero, ..00 ffffffff carries into byte 11, ff..fe wraps at
// the second increment).  The message buffer holds exactly nproofs * L bytes on the heap, so a lane of the partial block that reads past byte L is a sanitizer report;
// guard bytes lie behind the traces.  Checked per proof: every row of (A z) o (B z) = C z holds; the instance is One, the icb bits, the bits of zkaes_ctr_crypt's
// ciphertext, zero padding; flipping one ciphertext bit of the instance leaves exactly one row unsatisfied, flipping one icb bit at least one.  No GPU: what the device
// adds is the launch.
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
static void counter(uint8_t out[16], int which, unsigned seed) {
    memset(out, 0, 16);
    switch (which) {
    case 0: memset(out, 0xff, 16); break;                                   // ff..ff: the first increment wraps to zero
    case 1: memset(out + 12, 0xff, 4); break;                               // ..00 ffffffff: the carry reaches byte 11 (GCM's inc32 would not)
    case 2: memset(out, 0xff, 16); out[15] = 0xfe; break;                   // ff..fe: wraps at the second increment
    case 3: memset(out + 11, 0xff, 5); out[11] = 0x7f; break;               // ..7f ffffffff: the carry stops inside a byte
    case 4: out[15] = 0xff; break;                                          // ..00ff
    default: srand(seed); for (int i = 0; i < 16; i++) out[i] = (uint8_t)rand();
    }
}
int main() {
    uint8_t sb[256]; for (int i = 0; i < 256; i++) sb[i] = aes_sbox_value((uint8_t)i);
    int bad_total = 0;
    const size_t lens[5] = {1, 16, 17, 33, 48};
    const int ctrs[5][2] = {{5, 0}, {4, 5}, {0, 1}, {2, 3}, {1, 0}};
    for (int shape = 0; shape < 5; shape++) {
        const size_t L = lens[shape], nb = (L + 15) / 16;
        Circuit c = compile_aes_ctr_circuit(L);
        if (c.trace_bytes != TR_CTR_BYTES(nb) || c.message_bytes != L || c.n_blocks != nb) { printf("L=%zu: circuit header is off\n", L); bad_total++; }
        const uint32_t nproofs = 2;
        std::unique_ptr<uint8_t[]> msgs(new uint8_t[L * nproofs]);          // exactly the bytes that exist
        std::vector<uint8_t> keys(16 * nproofs), icbs(16 * nproofs), trace(c.trace_bytes * nproofs + 64, 0xAA);
        srand(100 + shape); for (size_t i = 0; i < L * nproofs; i++) msgs[i] = (uint8_t)rand(); for (auto &x : keys) x = (uint8_t)rand();
        for (uint32_t p = 0; p < nproofs; p++) counter(&icbs[16 * p], ctrs[shape][p], 7 * shape + p);
        for (uint32_t t = 0; t < nproofs * (nb + 1) + 3; t++) {
            blockIdx.x = t;
            k_aes_trace_ctr(trace.data(), c.trace_bytes, msgs.get(), keys.data(), icbs.data(), nproofs, (uint32_t)nb, (uint32_t)L, sb);
        }
        for (size_t i = c.trace_bytes * nproofs; i < trace.size(); i++) if (trace[i] != 0xAA) { printf("write past the traces\n"); bad_total++; }
        for (uint32_t p = 0; p < nproofs; p++) {
            std::vector<uint8_t> z(c.num_variables());
            for (uint32_t i = 0; i < z.size(); i++) { blockIdx.x = i; k_witness_expand(z.data(), c.desc.data(), (uint32_t)z.size(), trace.data() + p * c.trace_bytes, c.sbox_in_off.data(), c.sbox_tmpl.data(), sb); }
            size_t bad = unsatisfied(c, z);
            std::unique_ptr<uint8_t[]> ct(new uint8_t[L]);
            if (zkaes_ctr_crypt(msgs.get() + L * p, L, keys.data() + 16 * p, icbs.data() + 16 * p, ct.get()) != 0) { printf("zkaes_ctr_crypt: %s\n", zkaes_last_error()); return 1; }
            size_t ibad = z[0] != 1, at = 1;
            for (int i = 0; i < 16; i++) for (int k = 0; k < 8; k++) ibad += z[at++] != ((icbs[16 * p + i] >> k) & 1);
            for (size_t i = 0; i < L; i++) for (int k = 0; k < 8; k++) ibad += z[at++] != ((ct[i] >> k) & 1);
            if (at != c.raw_instance) ibad++;
            for (; at < c.num_instance; at++) ibad += z[at] != 0;
            // the tail's own bytes beyond the message are zero, in the message slot and in C_b
            const uint8_t *tr = trace.data() + p * c.trace_bytes;
            for (size_t i = L; i < 16 * nb; i++)
                ibad += tr[TR_BLOCK0 + (i / 16) * TR_BLOCK_STRIDE + TR_BL_MSG + i % 16] != 0 || tr[TR_CTR(nb) + TR_CTR_BLOCK0 + (i / 16) * TR_CTR_BLOCK_STRIDE + TR_CTR_BL_CT + i % 16] != 0;
            std::vector<uint8_t> zf(z);
            zf[129 + 8 * (L - 1) + 2] ^= 1;                                   // a ciphertext bit in the last (partial) byte
            size_t flip_ct = unsatisfied(c, zf);
            zf = z; zf[1 + 8 * 15] ^= 1;                                      // counter bit 0
            size_t flip_icb = unsatisfied(c, zf);
            printf("L=%zu proof %u: unsatisfied %zu, instance mismatches %zu, rows unsatisfied after a ciphertext flip %zu, after an icb flip %zu\n", L, p, bad, ibad, flip_ct, flip_icb);
            bad_total += (int)(bad + ibad) + (flip_ct != 1) + (flip_icb < 1);
        }
    }
    printf("total bad %d\n", bad_total);
    return bad_total != 0;
}
