// tests/keysize_trace_emu.cpp -- the trace kernels of csrc/kernels_witness.cuh instantiated for NK = 6 and 8 (AES-192, AES-256) and k_witness_expand, run lane by lane ON
// THE HOST: tests/test_keysize_host.py builds this file, which includes that header behind tests/lane_emu.h, with
// -fsanitize=address,undefined.  Shapes per key size: ECB nb = 1 and 2, CBC nb = 2, CTR L = 17 under the counter ff..ff (it wraps at the one increment), GCM (L, A) =
// (17, 5) and (1, 0); two proofs with different keys per launch.  The message, key and header buffers hold exactly the bytes that exist, on the heap, so a lane that
// reads a key at the AES-128 stride, or past a partial block, is a sanitizer report; guard bytes lie behind the traces, whose size is the layout macros' for that NK.
// Checked per proof: every row of (A z) o (B z) = C z holds; the instance is One, the public bits of the host cipher's output for that key length, zero padding; one
// flipped ciphertext bit leaves exactly one row unsatisfied; one flipped bit of the LAST key byte (byte 4 NK - 1: the second half of a 256-bit key) leaves at least one
// row unsatisfied.  Lanes beyond the grid return without writing.  No GPU: what the device adds is the launch.
#include "circuit.hpp"
#include "trace_layout.h"
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

// one launch: every lane of the grid, then three surplus lanes, which must leave the trace as it is
template <int NK>
static void launch(Mode mode, std::vector<uint8_t> &trace, size_t stride, const uint8_t *msgs, const uint8_t *keys, const uint8_t *pub, uint32_t nproofs, size_t nb, size_t na, size_t L, size_t A,
                   int &bad_total) {
    const uint32_t lanes = nproofs * (uint32_t)(mode == GCM ? nb + 3 : nb + 1), ghash_lanes = nproofs * (uint32_t)(na + nb + 2) * 16;
    std::vector<uint8_t> before;
    for (uint32_t t = 0; t < lanes + 3; t++) {
        if (t == lanes) before = trace;
        blockIdx.x = t;
        if (mode == ECB) k_aes_trace<false, NK>(trace.data(), stride, msgs, keys, nullptr, nproofs, (uint32_t)nb, sb);
        else if (mode == CBC) k_aes_trace<true, NK>(trace.data(), stride, msgs, keys, pub, nproofs, (uint32_t)nb, sb);
        else if (mode == CTR) k_aes_trace_ctr<NK>(trace.data(), stride, msgs, keys, pub, nproofs, (uint32_t)nb, (uint32_t)L, sb);
        else k_aes_trace_gcm<NK>(trace.data(), stride, msgs, keys, pub, nproofs, (uint32_t)nb, (uint32_t)na, (uint32_t)L, (uint32_t)A, sb);
    }
    bool quiet = before == trace;
    if (mode == GCM) {
        for (uint32_t t = 0; t < ghash_lanes + 3; t++) {
            if (t == ghash_lanes) before = trace;
            blockIdx.x = t;
            k_ghash_trace<NK>(trace.data(), stride, nproofs, (uint32_t)nb, (uint32_t)na, (uint32_t)L, (uint32_t)A);
        }
        quiet = quiet && before == trace;
    }
    if (quiet) printf("NK=%d %s: surplus lanes wrote nothing\n", NK, mode_name[mode]);
    else { printf("NK=%d %s: a lane beyond the grid wrote to the trace\n", NK, mode_name[mode]); bad_total++; }
}

template <int NK>
static void run(Mode mode, size_t L, size_t A, int &bad_total) {
    const size_t kb = 4 * NK, nb = (L + 15) / 16, na = (A + 15) / 16, hs = 12 + A;
    Circuit c = mode == ECB ? compile_aes_circuit(L, 8 * kb) : mode == CBC ? compile_aes_cbc_circuit(L, 8 * kb) : mode == CTR ? compile_aes_ctr_circuit(L, 8 * kb) : compile_aes_gcm_circuit(L, A, 8 * kb);
    const size_t want_bytes = mode == ECB ? TRK_ECB_BYTES(NK, nb) : mode == CBC ? TRK_CBC_BYTES(NK, nb) : mode == CTR ? TRK_CTR_BYTES(NK, nb) : TRK_GCM_BYTES(NK, na, nb);
    if (c.trace_bytes != want_bytes || c.key_bytes != kb || c.n_blocks != nb || c.sbox_in_off.size() != TRK_SBOX_KS(NK) + (mode == GCM ? nb + 2 : nb) * TRK_SBOX_PER_BLOCK(NK)) {
        printf("NK=%d %s L=%zu A=%zu: circuit header is off\n", NK, mode_name[mode], L, A); bad_total++;
    }
    const uint32_t nproofs = 2;
    const size_t pub_each = mode == GCM ? hs : 16;                                                  // the iv (CBC), the initial counter block (CTR), iv then aad (GCM)
    std::unique_ptr<uint8_t[]> msgs(new uint8_t[L * nproofs]), keys(new uint8_t[kb * nproofs]), pub(new uint8_t[pub_each * nproofs]);      // exactly the bytes that exist
    std::vector<uint8_t> trace(c.trace_bytes * nproofs + 64, 0xAA);
    srand(1000 * NK + 10 * (unsigned)mode + (unsigned)L);
    for (size_t i = 0; i < L * nproofs; i++) msgs[i] = (uint8_t)rand();
    for (size_t i = 0; i < kb * nproofs; i++) keys[i] = (uint8_t)rand();                             // two different keys
    for (size_t i = 0; i < pub_each * nproofs; i++) pub[i] = mode == CTR ? 0xff : (uint8_t)rand();
    launch<NK>(mode, trace, c.trace_bytes, msgs.get(), keys.get(), pub.get(), nproofs, nb, na, L, A, bad_total);
    for (size_t i = c.trace_bytes * nproofs; i < trace.size(); i++) if (trace[i] != 0xAA) { printf("write past the traces\n"); bad_total++; break; }
    for (uint32_t p = 0; p < nproofs; p++) {
        const uint8_t *tr = trace.data() + p * c.trace_bytes, *key = keys.get() + kb * p, *msg = msgs.get() + L * p, *pb = pub.get() + pub_each * p;
        std::vector<uint8_t> z(c.num_variables());
        for (uint32_t i = 0; i < z.size(); i++) { blockIdx.x = i; k_witness_expand(z.data(), c.desc.data(), (uint32_t)z.size(), tr, c.sbox_in_off.data(), c.sbox_tmpl.data(), sb); }
        size_t bad = unsatisfied(c, z);
        // the instance against the host cipher for this key length
        std::vector<uint8_t> ct(L), want_pub;
        uint8_t tag[16];
        if (mode == ECB) aes_ecb_encrypt_host(msg, L, key, kb, ct.data());
        else if (mode == CBC) aes128_cbc_encrypt_host(msg, L, key, pb, ct.data(), kb);
        else if (mode == CTR) aes128_ctr_crypt_host(msg, L, key, pb, ct.data(), kb);
        else aes128_gcm_encrypt_host(msg, L, key, pb, A ? pb + 12 : nullptr, A, ct.data(), tag, kb);
        if (mode != ECB) want_pub.assign(pb, pb + pub_each);
        const size_t ct_at = 1 + 8 * want_pub.size();
        want_pub.insert(want_pub.end(), ct.begin(), ct.end());
        if (mode == GCM) want_pub.insert(want_pub.end(), tag, tag + 16);
        size_t ibad = z[0] != 1, at = 1;
        for (uint8_t b : want_pub) for (int k = 0; k < 8; k++) ibad += z[at++] != ((b >> k) & 1);
        if (at != c.raw_instance) ibad++;
        for (; at < c.num_instance; at++) ibad += z[at] != 0;
        // the key bytes in the trace and the last round's state are where the layout says
        ibad += memcmp(tr + TR_KEY, key, kb) != 0;
        if (mode == ECB || mode == CBC) for (size_t b = 0; b < nb; b++) ibad += memcmp(tr + TRK_BLOCK0(NK) + b * TRK_BLOCK_STRIDE(NK) + TRK_BL_CT(NK), ct.data() + 16 * b, 16) != 0;
        std::vector<uint8_t> zf(z);
        zf[ct_at + 8 * (L - 1) + 2] ^= 1;                                                           // a bit of the last ciphertext byte
        size_t flip_ct = unsatisfied(c, zf);
        zf = z;
        zf[c.num_instance + 8 * L + 8 * (kb - 1) + 5] ^= 1;                                          // the witnesses are the message bits, then the key bits: bit 5 of key byte 4 NK - 1
        size_t flip_key = unsatisfied(c, zf);
        printf("NK=%d %s L=%zu A=%zu proof %u: unsatisfied %zu, instance mismatches %zu, rows unsatisfied after a ciphertext flip %zu, after a flip of the last key byte %zu\n", NK, mode_name[mode],
               L, A, p, bad, ibad, flip_ct, flip_key);
        bad_total += (int)(bad + ibad) + (flip_ct != 1) + (flip_key < 1);
    }
}

template <int NK>
static void run_all(int &bad_total) {
    run<NK>(ECB, 16, 0, bad_total);
    run<NK>(ECB, 32, 0, bad_total);
    run<NK>(CBC, 32, 0, bad_total);
    run<NK>(CTR, 17, 0, bad_total);
    run<NK>(GCM, 17, 5, bad_total);
    run<NK>(GCM, 1, 0, bad_total);
}

int main() {
    for (int i = 0; i < 256; i++) sb[i] = aes_sbox_value((uint8_t)i);
    int bad_total = 0;
    run_all<6>(bad_total);
    run_all<8>(bad_total);
    printf("total bad %d\n", bad_total);
    return bad_total != 0;
}
