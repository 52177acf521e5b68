// csrc/kernels_witness.hip -- R1CS witness generation for the reference's AES circuit and the sparse matrix products.
//
// Replaces the value side of the gadget synthesis in the reference's src/lib.rs:176-293 and src/aes_circuit.rs:20-427 (every UInt8/Boolean op there both allocates a
// variable and computes its value on the CPU).  Two layers:
//   the byte-typed trace   k_aes_trace, k_aes_trace_ctr, k_aes_trace_gcm, k_ghash_trace, their _seg forms, k_key_tag_trace and k_witness_expand live in
//                     kernels_witness.cuh, which only this file compiles for the device (the host emulators of tests/ include it too).  Here are their launchers: the
//                     argument checks, the S-box table's upload, the dispatch on the key size and the launch;
//   the field-typed kernels, in this file:
//   k_spmv_bits       z_A = A z, z_B = B z over 0/1 assignments with small integer coefficients (ark-marlin prover_init),
//   k_w_*, k_lagrange_finish, k_bits_to_field   the witness polynomial's evaluations and the Lagrange scalars of round 1,
//   k_t_evals         the round-2 "t" accumulation through a column-bucketed copy of A, B, C.
#include <mutex>
#include <type_traits>
#include "hip_util.hpp"
#include "kernels_witness.cuh"

namespace zk {
namespace gpu {

#define GRID(n) dim3((unsigned)(((n) + 255) / 256)), dim3(256)

// device copies of the S-box table, one per HIP device (keys on several GPUs of one process each use their own)
static uint8_t *g_sbox_dev[64] = {nullptr};
static std::mutex g_sbox_mu;
static int sbox_device() {
    int d = 0;
    HIP_CHECK(hipGetDevice(&d));
    if (d < 0 || d >= 64) throw GpuError("device ordinal out of range");
    return d;
}
void upload_sbox(const uint8_t table[256]) {
    const int d = sbox_device();
    std::lock_guard<std::mutex> g(g_sbox_mu);
    if (!g_sbox_dev[d]) g_sbox_dev[d] = (uint8_t *)dmalloc(256);      // lives for the life of the process (one table per device)
    HIP_CHECK(hipMemcpy(g_sbox_dev[d], table, 256, hipMemcpyHostToDevice));
}
// this device's table, for a launcher that cannot run without it
static uint8_t *sbox_required(const char *who) {
    const int d = sbox_device();
    std::lock_guard<std::mutex> g(g_sbox_mu);
    if (!g_sbox_dev[d]) throw GpuError(std::string(who) + ": S-box table not uploaded on this device");
    return g_sbox_dev[d];
}

// the launchers' view of the key size: 16, 24 or 32 key bytes -> NK, which the layout macros take as plain arithmetic and the kernels as a template argument
static int trace_nk(const char *who, size_t key_bytes) {
    if (key_bytes != 16 && key_bytes != 24 && key_bytes != 32) throw GpuError(std::string(who) + ": the AES key must have 16, 24 or 32 bytes");
    return (int)(key_bytes / 4);
}
// f(std::integral_constant<int, NK>) for the run-time nk = 4, 6 or 8 (trace_nk admits no other)
template <typename Fn>
static void dispatch_nk(int nk, Fn f) {
    if (nk == 4) f(std::integral_constant<int, 4>());
    else if (nk == 6) f(std::integral_constant<int, 6>());
    else f(std::integral_constant<int, 8>());
}

template <bool CBC>
static void launch_aes_trace(const char *who, uint8_t *trace, size_t stride, const uint8_t *msgs, const uint8_t *keys, const uint8_t *ivs, uint32_t nproofs, uint32_t nblocks, size_t key_bytes, stream_t s) {
    // the stride must hold the trace of THIS key size: a caller that sized its buffer for another one gets an error here, never lanes that store past a trace
    const int nk = trace_nk(who, key_bytes);
    const size_t need = CBC ? TRK_CBC_BYTES(nk, (size_t)nblocks) : TRK_ECB_BYTES(nk, (size_t)nblocks);
    if (stride < need) throw GpuError(std::string(who) + ": trace stride " + std::to_string(stride) + " is short of the " + std::to_string(need) + " bytes a " + std::to_string(8 * key_bytes) + "-bit key's trace takes");
    uint8_t *sbox = sbox_required(who);
    dispatch_nk(nk, [&](auto NK) { launch_lanes(k_aes_trace<CBC, decltype(NK)::value>, nproofs * (nblocks + 1), s, trace, stride, msgs, keys, ivs, nproofs, nblocks, sbox); });
}
void aes_trace(uint8_t *trace, size_t stride, const uint8_t *msgs, const uint8_t *keys, uint32_t nproofs, uint32_t nblocks, stream_t s, size_t key_bytes) {
    launch_aes_trace<false>("aes_trace", trace, stride, msgs, keys, nullptr, nproofs, nblocks, key_bytes, s);
}
void aes_trace_cbc(uint8_t *trace, size_t stride, const uint8_t *msgs, const uint8_t *keys, const uint8_t *ivs, uint32_t nproofs, uint32_t nblocks, stream_t s, size_t key_bytes) {
    if (!ivs) throw GpuError("aes_trace_cbc: no IV buffer");
    launch_aes_trace<true>("aes_trace_cbc", trace, stride, msgs, keys, ivs, nproofs, nblocks, key_bytes, s);
}
void aes_trace_ctr(uint8_t *trace, size_t stride, const uint8_t *msgs, const uint8_t *keys, const uint8_t *icbs, uint32_t nproofs, uint32_t msg_len, stream_t s, size_t key_bytes) {
    if (!icbs) throw GpuError("aes_trace_ctr: no counter buffer");
    if (msg_len == 0 || msg_len > 0xfffffff0u) throw GpuError("aes_trace_ctr: the message length must be 1 .. 2^32 - 16 bytes");
    const int nk = trace_nk("aes_trace_ctr", key_bytes);
    uint32_t nblocks = (msg_len + 15) / 16;
    if (stride < TRK_CTR_BYTES(nk, (size_t)nblocks)) throw GpuError("aes_trace_ctr: trace stride is short of the CTR tail");
    uint8_t *sbox = sbox_required("aes_trace_ctr");
    dispatch_nk(nk, [&](auto NK) { launch_lanes(k_aes_trace_ctr<decltype(NK)::value>, nproofs * (nblocks + 1), s, trace, stride, msgs, keys, icbs, nproofs, nblocks, msg_len, sbox); });
}
// what the GCM entries, whole records and segments, check alike: the lengths (and from them the block counts); then the stride against the trace's size for the key
// size and shape, 16-byte alignment (the GHASH lanes store 16 bytes at a time) and the proof count
static void gcm_lengths(const char *who, uint32_t msg_len, uint32_t aad_len, uint32_t &nblocks, uint32_t &naad) {
    if (msg_len == 0 || msg_len > (1u << 16) || aad_len > (1u << 16)) throw GpuError(std::string(who) + ": the message must have 1 .. 65536 bytes, the aad at most 65536");
    nblocks = (msg_len + 15) / 16; naad = (aad_len + 15) / 16;
}
static void gcm_trace_fits(const char *who, const uint8_t *trace, size_t stride, uint32_t nproofs, size_t need, const char *what) {
    if (stride < need) throw GpuError(std::string(who) + ": trace stride is short of the " + what);
    if (stride % 16 || (uintptr_t)trace % 16) throw GpuError(std::string(who) + ": traces must be 16-byte aligned");
    if (nproofs == 0 || nproofs > (1u << 20)) throw GpuError(std::string(who) + ": 1 .. 2^20 proofs per launch");
}
static int gcm_shape(const char *who, const uint8_t *trace, size_t stride, uint32_t nproofs, uint32_t msg_len, uint32_t aad_len, size_t key_bytes, uint32_t &nblocks, uint32_t &naad) {
    const int nk = trace_nk(who, key_bytes);
    gcm_lengths(who, msg_len, aad_len, nblocks, naad);
    gcm_trace_fits(who, trace, stride, nproofs, TRK_GCM_BYTES(nk, (size_t)naad, (size_t)nblocks), "GCM tail");
    return nk;
}
void aes_trace_gcm(uint8_t *trace, size_t stride, const uint8_t *msgs, const uint8_t *keys, const uint8_t *hdrs, uint32_t nproofs, uint32_t msg_len, uint32_t aad_len, stream_t s, size_t key_bytes) {
    if (!hdrs) throw GpuError("aes_trace_gcm: no iv / aad buffer");
    uint32_t nblocks, naad;
    const int nk = gcm_shape("aes_trace_gcm", trace, stride, nproofs, msg_len, aad_len, key_bytes, nblocks, naad);
    uint8_t *sbox = sbox_required("aes_trace_gcm");
    dispatch_nk(nk, [&](auto NK) { launch_lanes(k_aes_trace_gcm<decltype(NK)::value>, nproofs * (nblocks + 3), s, trace, stride, msgs, keys, hdrs, nproofs, nblocks, naad, msg_len, aad_len, sbox); });
}
void ghash_trace(uint8_t *trace, size_t stride, uint32_t nproofs, uint32_t msg_len, uint32_t aad_len, stream_t s, size_t key_bytes) {
    uint32_t nblocks, naad;
    const int nk = gcm_shape("ghash_trace", trace, stride, nproofs, msg_len, aad_len, key_bytes, nblocks, naad);
    dispatch_nk(nk, [&](auto NK) { launch_lanes(k_ghash_trace<decltype(NK)::value>, nproofs * (naad + nblocks + 2) * 16, s, trace, stride, nproofs, nblocks, naad, msg_len, aad_len); });
}
// what the segment entries check before any lane runs: the role, the key size, the lengths by role, and the stride and alignment against the segment trace's size
static int gcm_seg_shape(const char *who, const uint8_t *trace, size_t stride, uint32_t nproofs, int role, uint32_t msg_len, uint32_t aad_len, size_t key_bytes, uint32_t &nblocks, uint32_t &naad) {
    const int nk = trace_nk(who, key_bytes);
    if (role != TRS_HEAD && role != TRS_MID && role != TRS_TAIL && role != TRS_LAST) throw GpuError(std::string(who) + ": the role must be 0 (head), 1 (mid), 2 (tail) or 3 (last)");
    // (a tail of 0 bytes is the closing tail of a digest record, DESIGN.md 9m: no data block, nblocks = 0)
    if (role == TRS_TAIL && msg_len == 0) {
        if (aad_len > (1u << 16)) throw GpuError(std::string(who) + ": the aad has at most 65536 bytes");
        nblocks = 0; naad = (aad_len + 15) / 16;
    } else gcm_lengths(who, msg_len, aad_len, nblocks, naad);
    if (role != TRS_TAIL && role != TRS_LAST && msg_len % 16) throw GpuError(std::string(who) + ": a head or mid segment takes whole blocks");
    if (role != TRS_HEAD && aad_len) throw GpuError(std::string(who) + ": only a head segment takes aad");
    if (!trace) throw GpuError(std::string(who) + ": no trace buffer");
    gcm_trace_fits(who, trace, stride, nproofs, TRS_BYTES(nk, role, (size_t)naad, (size_t)nblocks), "segment region");
    return nk;
}
void aes_trace_gcm_seg(uint8_t *trace, size_t stride, const uint8_t *msgs, const uint8_t *keys, const uint8_t *hdrs, uint32_t nproofs, int role, uint32_t msg_len, uint32_t aad_len, stream_t s, size_t key_bytes) {
    if (!msgs || !keys || !hdrs) throw GpuError("aes_trace_gcm_seg: no message, key or header buffer");
    uint32_t nblocks, naad;
    const int nk = gcm_seg_shape("aes_trace_gcm_seg", trace, stride, nproofs, role, msg_len, aad_len, key_bytes, nblocks, naad);
    uint8_t *sbox = sbox_required("aes_trace_gcm_seg");
    dispatch_nk(nk, [&](auto NK) {
        launch_lanes(k_aes_trace_gcm_seg<decltype(NK)::value>, nproofs * (TRS_SLOTS(role, nblocks) + 1), s, trace, stride, msgs, keys, hdrs, nproofs, (uint32_t)role, nblocks, naad, msg_len, aad_len, sbox);
    });
}
void ghash_trace_seg(uint8_t *trace, size_t stride, uint32_t nproofs, int role, uint32_t msg_len, uint32_t aad_len, stream_t s, size_t key_bytes) {
    uint32_t nblocks, naad;
    const int nk = gcm_seg_shape("ghash_trace_seg", trace, stride, nproofs, role, msg_len, aad_len, key_bytes, nblocks, naad);
    dispatch_nk(nk, [&](auto NK) { launch_lanes(k_ghash_trace_seg<decltype(NK)::value>, nproofs * (TRS_MULS(role, naad, nblocks) + 1) * 16, s, trace, stride, nproofs, (uint32_t)role, nblocks, naad); });
}
// what the entry checks before any lane runs: T, the slots inside the stride, and 16-byte alignment of slot 0 and of every trace (as the GCM entries: tagged traces are
// 16-byte multiples for every mode and key size)
void key_tag_trace(uint8_t *trace, size_t stride, size_t tag_off, const uint8_t *keys, uint32_t nproofs, uint32_t tag_blocks, stream_t s, size_t key_bytes) {
    const int nk = trace_nk("key_tag_trace", key_bytes);
    if (!trace || !keys) throw GpuError("key_tag_trace: no trace or key buffer");
    if (tag_blocks != 1 && tag_blocks != 2) throw GpuError("key_tag_trace: 1 or 2 tag blocks");
    const size_t slot = TRK_BLOCK_STRIDE(nk);
    if (tag_off < (size_t)TRK_BLOCK0(nk) || tag_off > stride || stride - tag_off < tag_blocks * slot)
        throw GpuError("key_tag_trace: trace stride " + std::to_string(stride) + " does not hold " + std::to_string(tag_blocks) + " tag slots of " + std::to_string(slot) + " bytes at offset " + std::to_string(tag_off));
    if (tag_off % 16 || stride % 16 || (uintptr_t)trace % 16) throw GpuError("key_tag_trace: tagged traces and the tag offset must be 16-byte aligned");
    if (nproofs == 0 || nproofs > (1u << 20)) throw GpuError("key_tag_trace: 1 .. 2^20 proofs per launch");
    uint8_t *sbox = sbox_required("key_tag_trace");
    dispatch_nk(nk, [&](auto NK) { launch_lanes(k_key_tag_trace<decltype(NK)::value>, nproofs * tag_blocks, s, trace, stride, tag_off, keys, nproofs, tag_blocks, sbox); });
}

void witness_expand(uint8_t *z, const uint32_t *desc, uint32_t ncols, const uint8_t *trace, const uint32_t *sbox_in_off, const uint32_t *sbox_tmpl, stream_t s) {
    hipLaunchKernelGGL(k_witness_expand, GRID(ncols), 0, (hipStream_t)s, z, desc, ncols, trace, sbox_in_off, sbox_tmpl, sbox_required("witness_expand"));
    HIP_LAUNCH_CHECK();
}

__device__ __forceinline__ F small_to_field(long long v) { return F::from_i64(v); }

__global__ void k_spmv_bits(F *__restrict__ out, int8_t *__restrict__ small_out, size_t rows_out, const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ col, const int64_t *__restrict__ coeff,
                            size_t rows, const uint8_t *__restrict__ z) {
    size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows_out) return;
    long long acc = 0;
    if (r < rows) for (uint32_t i = rowptr[r]; i < rowptr[r + 1]; i++) acc += z[col[i]] ? coeff[i] : 0;
    out[r] = acc == 0 ? F::zero() : small_to_field(acc);
    if (small_out) small_out[r] = (int8_t)(acc > 127 ? 127 : (acc < -127 ? -127 : acc));
}
void spmv_bits(F *out, int8_t *small_out, size_t rows_out, const uint32_t *rowptr, const uint32_t *col, const int64_t *coeff, size_t rows, const uint8_t *z, stream_t s) {
    hipLaunchKernelGGL(k_spmv_bits, GRID(rows_out), 0, (hipStream_t)s, out, small_out, rows_out, rowptr, col, coeff, rows, z); HIP_LAUNCH_CHECK();
}
__global__ void k_w_classes(int8_t *__restrict__ out, const uint8_t *__restrict__ z, uint32_t n, uint32_t m, uint32_t num_witness) {
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    uint32_t ratio = n / m;
    if (k % ratio == 0) { out[k] = 0; return; }
    uint32_t wi = k - k / ratio - 1;
    out[k] = (wi < num_witness && z[m + wi]) ? 1 : 0;
}
void w_classes(int8_t *out, const uint8_t *z, uint32_t n, uint32_t m, uint32_t num_witness, stream_t s) {
    hipLaunchKernelGGL(k_w_classes, GRID(n), 0, (hipStream_t)s, out, z, n, m, num_witness); HIP_LAUNCH_CHECK();
}
__global__ void k_lagrange_finish(F *__restrict__ lag, F *__restrict__ lag_w, const F *__restrict__ elems, uint32_t n, uint32_t m, F vx_inv, F n_inv) {
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    F v = lag[k] * (elems[k] * n_inv);  // lag[k] arrives as (beta^n - 1) / (beta - g^k)
    lag[k] = v;
    lag_w[k] = (k % (n / m) == 0) ? F::zero() : v * vx_inv;
}
void lagrange_scalars(F *lag, F *lag_w, const F *elems, const F &beta, uint32_t n, uint32_t m, stream_t s) {
    int lg_n = 0;
    while ((1u << lg_n) < n) lg_n++;
    F vx_inv = (beta.pow_u64(m) - F::one()).inverse();
    // (beta^n - 1) / (beta - g^k) = r(beta, g^k): the product tree of kernels_poly.hip (no batch inversion)
    const size_t need = vanishing_quotient_scratch(lg_n, 1);
    DevPtr<F> scratch(need);
    F *outs[1] = {lag};
    const F one = F::one();
    vanishing_quotient_evals(outs, &one, 1, beta, elems, n, lg_n, scratch, need, s);
    hipLaunchKernelGGL(k_lagrange_finish, GRID(n), 0, (hipStream_t)s, lag, lag_w, elems, n, m, vx_inv, F::from_u64(n).inverse()); HIP_LAUNCH_CHECK();
    sync(s);                            // (the scratch is released on return)
}

__global__ void k_w_evals(F *__restrict__ out, const uint8_t *__restrict__ z, const F *__restrict__ x_evals, uint32_t n, uint32_t m, uint32_t num_witness) {
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    uint32_t ratio = n / m;
    if (k % ratio == 0) { out[k] = F::zero(); return; }
    uint32_t wi = k - k / ratio - 1;
    F w = (wi < num_witness && z[m + wi]) ? F::one() : F::zero();
    out[k] = w - x_evals[k];
}
void w_evals(F *out, const uint8_t *z, const F *x_evals, uint32_t n, uint32_t m, uint32_t num_witness, stream_t s) {
    hipLaunchKernelGGL(k_w_evals, GRID(n), 0, (hipStream_t)s, out, z, x_evals, n, m, num_witness); HIP_LAUNCH_CHECK();
}
__global__ void k_bits_to_field(F *__restrict__ out, const uint8_t *__restrict__ z, size_t n) { size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; if (i < n) out[i] = z[i] ? F::one() : F::zero(); }
void bits_to_field(F *out, const uint8_t *z, size_t n, stream_t s) { if (!n) return; hipLaunchKernelGGL(k_bits_to_field, GRID(n), 0, (hipStream_t)s, out, z, n); HIP_LAUNCH_CHECK(); }

// Two passes so that heavy columns (the constant One, key bits) do not serialize on one lane: pass 1 = one lane per SEGMENT of at most
// T_SEG entries of one column, pass 2 = one lane per column adding its segments' partial sums.
__global__ void k_t_partials(F *__restrict__ partial, uint32_t nseg, const uint32_t *__restrict__ seg_start, const uint32_t *__restrict__ seg_end, const uint32_t *__restrict__ row,
                             const uint8_t *__restrict__ mat, const int64_t *__restrict__ coeff, const F *__restrict__ r_alpha, F eta_a, F eta_b, F eta_c) {
    uint32_t sgi = blockIdx.x * blockDim.x + threadIdx.x;
    if (sgi >= nseg) return;
    F acc = F::zero();
    for (uint32_t i = seg_start[sgi]; i < seg_end[sgi]; i++) {
        F eta = mat[i] == 0 ? eta_a : (mat[i] == 1 ? eta_b : eta_c);
        long long c = coeff[i];
        F term = eta * r_alpha[row[i]];
        if (c == 1) acc = acc + term;
        else if (c == -1) acc = acc - term;
        else acc = acc + term * small_to_field(c);
    }
    partial[sgi] = acc;
}
// columns with more than T_HEAVY_SEGMENTS segments (the constant One, key bits) get a whole workgroup: k_t_heavy
__global__ void k_t_columns(F *__restrict__ out, uint32_t n, const uint32_t *__restrict__ col_seg_ptr, const F *__restrict__ partial) {
    uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= n) return;
    uint32_t a = col_seg_ptr[h], b = col_seg_ptr[h + 1];
    if (b - a > T_HEAVY_SEGMENTS) return;        // summed by k_t_heavy
    F acc = F::zero();
    for (uint32_t i = a; i < b; i++) acc = acc + partial[i];
    out[h] = acc;
}
__global__ void __launch_bounds__(256) k_t_heavy(F *__restrict__ out, const uint32_t *__restrict__ heavy, const uint32_t *__restrict__ col_seg_ptr, const F *__restrict__ partial) {
    __shared__ F sh[256];
    uint32_t h = heavy[blockIdx.x], t = threadIdx.x;
    F acc = F::zero();
    for (uint32_t i = col_seg_ptr[h] + t; i < col_seg_ptr[h + 1]; i += 256) acc = acc + partial[i];
    sh[t] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if ((int)t < s) sh[t] = sh[t] + sh[t + s]; __syncthreads(); }
    if (t == 0) out[h] = sh[0];
}
void t_evals(F *out, uint32_t n, F *partial, uint32_t nseg, const uint32_t *col_seg_ptr, const uint32_t *seg_start, const uint32_t *seg_end, const uint32_t *heavy, uint32_t n_heavy,
             const uint32_t *row, const uint8_t *mat, const int64_t *coeff, const F *r_alpha, const F &eta_a, const F &eta_b, const F &eta_c, stream_t s) {
    if (nseg) { hipLaunchKernelGGL(k_t_partials, GRID(nseg), 0, (hipStream_t)s, partial, nseg, seg_start, seg_end, row, mat, coeff, r_alpha, eta_a, eta_b, eta_c); HIP_LAUNCH_CHECK(); }
    hipLaunchKernelGGL(k_t_columns, GRID(n), 0, (hipStream_t)s, out, n, col_seg_ptr, partial); HIP_LAUNCH_CHECK();
    if (n_heavy) { hipLaunchKernelGGL(k_t_heavy, dim3(n_heavy), dim3(256), 0, (hipStream_t)s, out, heavy, col_seg_ptr, partial); HIP_LAUNCH_CHECK(); }
}

}  // namespace gpu
}  // namespace zk
