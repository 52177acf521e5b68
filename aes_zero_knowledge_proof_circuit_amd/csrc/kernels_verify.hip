// csrc/kernels_verify.hip -- the per-proof elliptic-curve and field work of the batch verifier (verify_batch.hpp) on gfx950: decompression and
// subgroup checks of the proofs' compressed G1 points, and the Lagrange evaluation x^(beta) of every proof's public input.  The two MSMs of a batch go through the
// variable-base MSM of kernels_msm.hip.
#include "hip_util.hpp"
#include "gpu.hpp"
#include "fq_sqrt.cuh"
#include "verify_batch.hpp"

namespace zk {
namespace gpu {

// One lane per point.  The square root's Tonelli-Shanks loop is data-dependent (lanes of a wave leave it at different rounds); the subgroup ladder behind it is driven
// by the bits of r, the same in every lane, so the lanes that reach it walk it together.  A lane whose x is not on the curve has nothing to multiply and waits.
__global__ void __launch_bounds__(64) k_g1_decompress_check(const G1Compressed *__restrict__ pts, uint32_t n, SqrtConsts K, Affine<Fq377> *__restrict__ out, uint8_t *__restrict__ status) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    uint32_t x[12];
#pragma unroll
    for (int k = 0; k < 12; k++) x[k] = pts[i].x[k];
    Affine<Fq377> a;
    status[i] = zk::g1_decompress_check(K, x, pts[i].y_gt != 0, a);
    out[i] = a;
}

// out[i] = sqrt(in[i]) (Montgomery limbs in and out), ok[i] = 0 for a non-residue (out[i] = 0 then)
__global__ void __launch_bounds__(64) k_fq_sqrt(const Fq377 *__restrict__ in, uint32_t n, SqrtConsts K, Fq377 *__restrict__ out, uint8_t *__restrict__ ok) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    Fq377 r = Fq377::zero();
    const bool sq = zk::fq_sqrt(K, in[i], r);
    out[i] = sq ? r : Fq377::zero();
    ok[i] = sq ? 1 : 0;
}

// x^(beta) = sum_j L_j(beta) x_j over the domain X = {g^j}, |X| = m = 2^lg_m, x = [1, the row's bits, zeros]; L_j(beta) = v_X(beta) g^j / (m (beta - g^j)).
// One workgroup per proof.  Every lane folds its set bits into ONE fraction N / D = sum_j g^j / (beta - g^j) (N <- N d + g^j D, D <- D d: no inversion per term), the
// workgroup adds its fractions in an LDS tree, and lane 0 inverts once.  When beta lies in X (v_X(beta) = 0) the basis is an indicator and the lane that owns
// g^j = beta writes x_j, as the host code does.  bits: rows of `words` 32-bit words, bit j - 1 of the row = x_j, LSB first.
constexpr int PIE_THREADS = 256;
__global__ void __launch_bounds__(PIE_THREADS) k_public_input_eval(const F *__restrict__ betas, const uint32_t *__restrict__ bits, uint32_t words, uint32_t n_bits, int lg_m, F gx, F m_inv,
                                                                   F *__restrict__ out) {
    __shared__ F shN[PIE_THREADS], shD[PIE_THREADS];
    const uint32_t p = blockIdx.x, t = threadIdx.x, m = 1u << lg_m;
    const F beta = betas[p];
    const uint32_t *row = bits + (size_t)p * words;
    F vx = beta;
    for (int k = 0; k < lg_m; k++) vx = vx.sqr();
    vx = vx - F::one();                                        // every lane computes v_X(beta): lg_m squarings, no broadcast needed
    const bool indicator = vx.is_zero();
    const F step = gx.pow_u64(PIE_THREADS);
    F e = gx.pow_u64(t), N = F::zero(), D = F::one();
    for (uint32_t j = t; j < m; j += PIE_THREADS, e = e * step) {
        const bool xj = j == 0 || (j - 1 < n_bits && ((row[(j - 1) >> 5] >> ((j - 1) & 31)) & 1));
        if (indicator) {
            if (e == beta) out[p] = xj ? F::one() : F::zero();
            continue;
        }
        if (!xj) continue;
        const F d = beta - e;
        N = N * d + e * D;
        D = D * d;
    }
    if (indicator) return;                                     // (uniform over the workgroup: beta is the block's own)
    shN[t] = N; shD[t] = D;
    __syncthreads();
    for (int h = PIE_THREADS / 2; h >= 1; h >>= 1) {
        if ((int)t < h) {
            const F n1 = shN[t], d1 = shD[t], n2 = shN[t + h], d2 = shD[t + h];
            shN[t] = n1 * d2 + n2 * d1;
            shD[t] = d1 * d2;
        }
        __syncthreads();
    }
    if (t == 0) out[p] = shN[0] * shD[0].inverse() * vx * m_inv;
}

// The keyed form: proofs of several verifying keys in one launch.  Proof p reads its key index, takes {lg_m, n_bits, gx, m_inv} from that key's
// descriptor and its packed bits from bits + row_word_off[p]: rows are ragged, ceil(n_bits / 32) words each, possibly none (a row without bits is never read).
// Everything behind the descriptor is k_public_input_eval's: lg_m is the block's own, so the indicator branch's early return stays uniform over the workgroup.
__global__ void __launch_bounds__(PIE_THREADS) k_public_input_eval_keyed(const F *__restrict__ betas, const uint32_t *__restrict__ bits, const uint32_t *__restrict__ key_of,
                                                                         const uint32_t *__restrict__ row_word_off, const PieKey *__restrict__ keys, F *__restrict__ out) {
    __shared__ F shN[PIE_THREADS], shD[PIE_THREADS];
    const uint32_t p = blockIdx.x, t = threadIdx.x;
    const PieKey *key = keys + key_of[p];
    const int lg_m = (int)key->lg_m;
    const uint32_t n_bits = key->n_bits, m = 1u << lg_m;
    const F gx = key->gx;
    const F beta = betas[p];
    const uint32_t *row = bits + row_word_off[p];
    F vx = beta;
    for (int k = 0; k < lg_m; k++) vx = vx.sqr();
    vx = vx - F::one();
    const bool indicator = vx.is_zero();
    const F step = gx.pow_u64(PIE_THREADS);
    F e = gx.pow_u64(t), N = F::zero(), D = F::one();
    for (uint32_t j = t; j < m; j += PIE_THREADS, e = e * step) {
        const bool xj = j == 0 || (j - 1 < n_bits && ((row[(j - 1) >> 5] >> ((j - 1) & 31)) & 1));
        if (indicator) {
            if (e == beta) out[p] = xj ? F::one() : F::zero();
            continue;
        }
        if (!xj) continue;
        const F d = beta - e;
        N = N * d + e * D;
        D = D * d;
    }
    if (indicator) return;                                     // (uniform over the workgroup: beta and the key are the block's own)
    shN[t] = N; shD[t] = D;
    __syncthreads();
    for (int h = PIE_THREADS / 2; h >= 1; h >>= 1) {
        if ((int)t < h) {
            const F n1 = shN[t], d1 = shD[t], n2 = shN[t + h], d2 = shD[t + h];
            shN[t] = n1 * d2 + n2 * d1;
            shD[t] = d1 * d2;
        }
        __syncthreads();
    }
    if (t == 0) out[p] = shN[0] * shD[0].inverse() * vx * key->m_inv;
}

void g1_decompress_check(const G1Compressed *pts, size_t n, Affine<Fq377> *out, uint8_t *status, stream_t s) {
    if (!n) return;
    if (n >= ((size_t)1 << 31)) throw GpuError("g1_decompress_check: too many points");
    hipLaunchKernelGGL(k_g1_decompress_check, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)s, pts, (uint32_t)n, sqrt_consts(), out, status);
    HIP_LAUNCH_CHECK();
}
void fq_sqrt_batch(const Fq377 *in, size_t n, Fq377 *out, uint8_t *ok, stream_t s) {
    if (!n) return;
    if (n >= ((size_t)1 << 31)) throw GpuError("fq_sqrt_batch: too many elements");
    hipLaunchKernelGGL(k_fq_sqrt, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)s, in, (uint32_t)n, sqrt_consts(), out, ok);
    HIP_LAUNCH_CHECK();
}
void public_input_eval(F *out, const F *betas, const uint32_t *bits, size_t words, size_t n, size_t n_bits, int lg_m, const F &gx, stream_t s) {
    if (!n) return;
    if (lg_m < 0 || lg_m > 30 || n >= ((size_t)1 << 31) || n_bits >= ((size_t)1 << lg_m) || words * 32 < n_bits || words >= ((size_t)1 << 26))
        throw GpuError("public_input_eval: the rows do not fit the domain");
    const F m_inv = F::from_u64((uint64_t)1 << lg_m).inverse();
    hipLaunchKernelGGL(k_public_input_eval, dim3((unsigned)n), dim3(PIE_THREADS), 0, (hipStream_t)s, betas, bits, (uint32_t)words, (uint32_t)n_bits, lg_m, gx, m_inv, out);
    HIP_LAUNCH_CHECK();
}
PieKey pie_key(int lg_m, size_t n_bits, const F &gx) {
    if (lg_m < 0 || lg_m > 30 || n_bits >= ((size_t)1 << lg_m)) throw GpuError("public_input_eval_keyed: the rows do not fit the domain");
    PieKey k;
    k.gx = gx;
    k.m_inv = F::from_u64((uint64_t)1 << lg_m).inverse();
    k.lg_m = (uint32_t)lg_m; k.n_bits = (uint32_t)n_bits;
    return k;
}
void public_input_eval_keyed(F *out, const F *betas, const uint32_t *bits, const uint32_t *key_of, const uint32_t *row_word_off, const PieKey *keys, const PieKeyedHost &h, size_t n, stream_t s) {
    if (!n) return;
    if (n >= ((size_t)1 << 31) || h.n_keys == 0 || h.n_keys >= ((size_t)1 << 31) || h.words >= ((size_t)1 << 31)) throw GpuError("public_input_eval_keyed: the rows do not fit the domain");
    for (size_t k = 0; k < h.n_keys; k++)
        if (h.keys[k].lg_m > 30 || h.keys[k].n_bits >= ((uint32_t)1 << h.keys[k].lg_m) || (h.keys[k].n_bits + 31) / 32 >= ((uint32_t)1 << 26)) throw GpuError("public_input_eval_keyed: the rows do not fit the domain");
    for (size_t p = 0; p < n; p++) {                           // every row lies inside the packed buffer: the kernel reads row_word_off[p] .. + ceil(n_bits / 32) and nothing else
        if (h.key_of[p] >= h.n_keys) throw GpuError("public_input_eval_keyed: key index out of range");
        const size_t w = (h.keys[h.key_of[p]].n_bits + 31) / 32;
        if ((size_t)h.row_word_off[p] > h.words || w > h.words - h.row_word_off[p]) throw GpuError("public_input_eval_keyed: a row lies outside the packed bits");
    }
    hipLaunchKernelGGL(k_public_input_eval_keyed, dim3((unsigned)n), dim3(PIE_THREADS), 0, (hipStream_t)s, betas, bits, key_of, row_word_off, keys, out);
    HIP_LAUNCH_CHECK();
}

}  // namespace gpu
}  // namespace zk
