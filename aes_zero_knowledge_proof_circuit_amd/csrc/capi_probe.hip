// csrc/capi_probe.hip -- zkaes_arith_probe: one field or curve operation per launch on raw limbs (TEST-ONLY; arith_probe.cuh, tests/test_gpu_arith.py)
#include "../../include/zkaes.h"
#include <stdexcept>
#include <string>
#include "hip_util.hpp"
#include "gpu.hpp"
#include "arith_probe.cuh"

// One kernel per operation: the operation is the template parameter, chosen on the host (a kernel holding every group law at once would spill).  One case per lane.
// The hot loop's bias and seed are taken at kernel entry, before any operand is loaded, as k_accumulate takes its seed.
template <class O> __global__ void __launch_bounds__(64) k_arith_probe(const uint32_t *__restrict__ in, uint32_t n_cases, uint32_t *__restrict__ out) {
    const uint64_t bias = zk::FpMsm<zk::Fq377P>::hot_loop_bias();
    const zk::FpMsm<zk::Fq377P>::Seed seed = zk::FpMsm<zk::Fq377P>::hot_loop_seed();
    const uint32_t c = blockIdx.x * 64 + threadIdx.x;
    if (c >= n_cases) return;
    uint32_t a[O::NIN], r[O::NOUT];
#pragma unroll
    for (int i = 0; i < O::NIN; i++) a[i] = in[(size_t)c * O::NIN + i];
    if constexpr (O::SEEDED) O::run_seeded(a, r, seed); else O::run(a, r, bias);
#pragma unroll
    for (int i = 0; i < O::NOUT; i++) out[(size_t)c * O::NOUT + i] = r[i];
}
// One case per FOUR lanes: lane q of the quad holds coordinate q.  The lanes of a quad share their case, so a quad is live or idle as a whole -- the callers in
// kernels_msm.hip run the quad forms under `if (active)` in the same way.
template <class O> __global__ void __launch_bounds__(64) k_arith_probe_quad(const uint32_t *__restrict__ in, uint32_t n_cases, uint32_t *__restrict__ out) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x, c = t >> 2;
    const int q = (int)(t & 3);
    if (c < n_cases) O::run_quad(in + (size_t)c * O::NIN, out + (size_t)c * O::NOUT, q);
}

extern "C" const char *zkaes_last_error(void);
namespace zk { void capi_set_error(const std::string &); }

namespace {
using zk::gpu::DevPtr; using zk::gpu::StreamGuard;
template <class O> void run_probe(const uint32_t *in, size_t n, uint32_t *out) {
    zk::gpu::require_device();
    StreamGuard s;
    DevPtr<uint32_t> din(n * O::NIN), dout(n * O::NOUT);
    zk::gpu::h2d(din, in, n * O::NIN * sizeof(uint32_t), s);
    hipStream_t hs = (hipStream_t)s.h;
    if constexpr (O::QUAD) k_arith_probe_quad<O><<<(unsigned)((4 * n + 63) / 64), 64, 0, hs>>>(din, (uint32_t)n, dout);
    else k_arith_probe<O><<<(unsigned)((n + 63) / 64), 64, 0, hs>>>(din, (uint32_t)n, dout);
    HIP_LAUNCH_CHECK();
    zk::gpu::d2h(out, dout, n * O::NOUT * sizeof(uint32_t), s);
}
}  // namespace

extern "C" int zkaes_arith_probe(int op, const uint32_t *in, size_t n_cases, uint32_t *out) {
    try {
        zk::capi_set_error("");
        if (!in || !out) throw std::invalid_argument("zkaes_arith_probe: null argument");
        if (n_cases == 0 || n_cases > zk::probe::MAX_CASES) throw std::invalid_argument("zkaes_arith_probe: n_cases must be in [1, 65536]");
        const auto run = [&](auto tag) { run_probe<typename decltype(tag)::type>(in, n_cases, out); };
        if (!zk::probe::dispatch(op, run) && !zk::probe::dispatch_zip(op, run)) throw std::invalid_argument("zkaes_arith_probe: unknown op " + std::to_string(op));
        return 0;
    } catch (const std::exception &e) { zk::capi_set_error(e.what()); return 1; }
    catch (...) { zk::capi_set_error("unknown error"); return 1; }
}
