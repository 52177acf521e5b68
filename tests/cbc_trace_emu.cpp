// tests/cbc_trace_emu.cpp -- the AES trace kernel (both modes) and k_witness_expand of csrc/kernels_witness.cuh run lane by lane ON THE HOST: tests/test_cbc_host.py builds
// this file, which includes that header behind tests/lane_emu.h, with -fsanitize=address,undefined.  For nb = 1, 2, 3 and two proofs per
// launch it checks that no lane writes outside the traces, that the expanded assignment satisfies every row of (A z) o (B z) = C z, that the instance is One, (the IV bits,)
// the bits of the host's own ciphertext and zero padding, and that flipping one instance bit leaves exactly one row unsatisfied.  No GPU: what the device adds is the launch.
#include "circuit.hpp"
#include "trace_layout.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "lane_emu.h"
#include "kernels_witness.cuh"
using namespace zk;
using namespace zk::gpu;
static long long rowdot(const CsrMatrix &m, size_t r, const std::vector<uint8_t> &z) { long long a = 0; for (uint32_t i = m.rowptr[r]; i < m.rowptr[r + 1]; i++) a += z[m.col[i]] ? m.coeff[i] : 0; return a; }
int main() {
    uint8_t sb[256]; for (int i = 0; i < 256; i++) sb[i] = aes_sbox_value((uint8_t)i);
    int bad_total = 0;
    for (size_t nb : {1, 2, 3}) for (int mode = 0; mode < 2; mode++) {
        Circuit c = mode ? compile_aes_cbc_circuit(16 * nb) : compile_aes_circuit(16 * nb);
        const uint32_t nproofs = 2;
        std::vector<uint8_t> msgs(16 * nb * nproofs), keys(16 * nproofs), ivs(16 * nproofs), trace(c.trace_bytes * nproofs + 64, 0xAA);
        srand(nb * 7 + mode); for (auto &x : msgs) x = rand(); for (auto &x : keys) x = rand(); for (auto &x : ivs) x = rand();
        for (uint32_t t = 0; t < nproofs * (nb + 1) + 3; t++) {
            blockIdx.x = t;
            if (mode) k_aes_trace<true>(trace.data(), c.trace_bytes, msgs.data(), keys.data(), ivs.data(), nproofs, (uint32_t)nb, sb);
            else k_aes_trace<false>(trace.data(), c.trace_bytes, msgs.data(), keys.data(), nullptr, nproofs, (uint32_t)nb, sb);
        }
        for (size_t i = c.trace_bytes * nproofs; i < trace.size(); i++) if (trace[i] != 0xAA) { printf("write past the traces\n"); bad_total++; }
        for (uint32_t p = 0; p < nproofs; p++) {
            std::vector<uint8_t> z(c.num_variables());
            for (uint32_t i = 0; i < z.size(); i++) { blockIdx.x = i; k_witness_expand(z.data(), c.desc.data(), (uint32_t)z.size(), trace.data() + p * c.trace_bytes, c.sbox_in_off.data(), c.sbox_tmpl.data(), sb); }
            size_t bad = 0;
            for (size_t r = 0; r < c.num_constraints; r++) if (rowdot(c.A, r, z) * rowdot(c.B, r, z) != rowdot(c.C, r, z)) bad++;
            // instance against the host chain
            std::vector<uint8_t> ct(16 * nb);
            uint8_t zero[16] = {0};
            if (mode) aes128_cbc_encrypt_host(msgs.data() + 16 * nb * p, 16 * nb, keys.data() + 16 * p, ivs.data() + 16 * p, ct.data());
            else for (size_t b = 0; b < nb; b++) aes128_cbc_encrypt_host(msgs.data() + 16 * (nb * p + b), 16, keys.data() + 16 * p, zero, ct.data() + 16 * b);
            size_t ibad = z[0] != 1, at = 1;
            if (mode) for (int i = 0; i < 16; i++) for (int k = 0; k < 8; k++) ibad += z[at++] != ((ivs[16 * p + i] >> k) & 1);
            for (size_t i = 0; i < 16 * nb; i++) for (int k = 0; k < 8; k++) ibad += z[at++] != ((ct[i] >> k) & 1);
            for (; at < c.num_instance; at++) ibad += z[at] != 0;
            // flip one IV bit / ct bit: exactly one row unsatisfied
            size_t flip_bad = 0;
            { std::vector<uint8_t> zf(z); zf[5] ^= 1; for (size_t r = 0; r < c.num_constraints; r++) if (rowdot(c.A, r, zf) * rowdot(c.B, r, zf) != rowdot(c.C, r, zf)) flip_bad++; }
            printf("nb=%zu mode=%s proof %u: unsatisfied %zu, instance mismatches %zu, rows unsatisfied after flipping instance bit 5: %zu\n", nb, mode ? "cbc" : "ecb", p, bad, ibad, flip_bad);
            bad_total += bad + ibad + (flip_bad != 1);
        }
    }
    printf("total bad %d\n", bad_total);
    return bad_total != 0;
}
