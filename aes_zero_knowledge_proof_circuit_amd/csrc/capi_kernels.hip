// csrc/capi_kernels.hip -- kernel-level C entry points (parity tests + roofline measurement) and device selection
#include "../../include/zkaes.h"
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>
#include "hip_util.hpp"
#include "marlin.hpp"
#include "marlin_host.hpp"
#include "te28.cuh"
#include <algorithm>
#include <chrono>

// stream-copy probe for the measured HBM peak bench.py prints next to the nominal 8 TB/s: 4 x 16 B per lane, all four loads
// issued before the first store, non-temporal both ways
typedef unsigned int v4u __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(256) k_stream_copy(uint4 *__restrict__ dst_, const uint4 *__restrict__ src_, size_t n16) {
    v4u *dst = (v4u *)dst_; const v4u *src = (const v4u *)src_;
    size_t base = (size_t)blockIdx.x * 1024 + threadIdx.x;
    if (base + 768 < n16) {
        v4u v0 = __builtin_nontemporal_load(src + base), v1 = __builtin_nontemporal_load(src + base + 256);
        v4u v2 = __builtin_nontemporal_load(src + base + 512), v3 = __builtin_nontemporal_load(src + base + 768);
        __builtin_nontemporal_store(v0, dst + base); __builtin_nontemporal_store(v1, dst + base + 256);
        __builtin_nontemporal_store(v2, dst + base + 512); __builtin_nontemporal_store(v3, dst + base + 768);
    } else {
        for (size_t i = base; i < n16; i += 256) dst[i] = src[i];
    }
}


// ---- per-box calibration of the integer roof (zkaes_int_rate_bench; bench.py prints it as roofline.int_multiplier.calibration).  Two probes, both bracketed per wave by
// s_memtime (shader-clock counter) and s_memrealtime (100 MHz): the isolated Fq377 reduced-radix product stream at four waves per SIMD -- what round 3's tools/ubench/rates.hip
// measured once on one box and every later bench line quoted -- and k_accumulate<EdwardsLaw>'s own loop (te_madd_hot) at the production launch shape over a table that stays
// in L2: the rate the hot kernel would run at on THIS box if its gathers were free.  Stamps: {shader cycles, real-time ticks} of lane 0 of every wave.
struct CalStamp { uint64_t cyc, rt; };
__global__ void __launch_bounds__(64) k_cal_fqmul(CalStamp *st, zk::FpMsm<zk::Fq377P> *sink, zk::FpMsm<zk::Fq377P> a, int iters) {
    using G = zk::FpMsm<zk::Fq377P>;
    const uint64_t bias = G::hot_loop_bias();
    G x = a, y = a;
    x.l[0] += threadIdx.x & 0xff;
    const uint64_t r0 = __builtin_amdgcn_s_memrealtime(), c0 = __builtin_readcyclecounter();
    for (int i = 0; i < iters; i++) { x = G::mul_biased(x, y, bias); y = G::mul_biased(y, x, bias); }
    const uint64_t c1 = __builtin_readcyclecounter(), r1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) { st[blockIdx.x].cyc = c1 - c0; st[blockIdx.x].rt = r1 - r0; }
    sink[blockIdx.x * 64 + threadIdx.x] = x + y;
}
__global__ void __launch_bounds__(64, 2) k_cal_hot_loop(CalStamp *st, zk::AccTE<zk::Fq377P> *sink, const zk::Niels28<zk::Fq377P> *__restrict__ tab, uint32_t mask, int iters) {
    using P = zk::Fq377P;
    const zk::FpMsm<P>::Seed seed = zk::FpMsm<P>::hot_loop_seed();
    uint32_t t = blockIdx.x * 64 + threadIdx.x, x = t * 2654435761u + 12345u;
    zk::AccTE<P> acc = zk::te_identity<P>();
    zk::Niels28<P> pt = zk::niels_load_signed<P>(tab + (x & mask), false);
    const uint64_t r0 = __builtin_amdgcn_s_memrealtime(), c0 = __builtin_readcyclecounter();
    for (int i = 0; i < iters; i++) {
        const uint32_t cur = x;
        x = x * 1664525u + 1013904223u;
        zk::te_madd_hot<P>(acc, pt, cur >> 31, tab + ((x >> 8) & mask), x >> 31, seed);
    }
    const uint64_t c1 = __builtin_readcyclecounter(), r1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) { st[blockIdx.x].cyc = c1 - c0; st[blockIdx.x].rt = r1 - r0; }
    sink[t] = acc;
}
__global__ void k_cal_fill(zk::Niels28<zk::Fq377P> *tab, uint32_t n) {       // arbitrary limbs < 2^28 stand in for curve points: the arithmetic is data-independent
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t x = i * 2654435761u + 99u;
    zk::Niels28<zk::Fq377P> r;
    for (int k = 0; k < 14; k++) { x = x * 1664525u + 1013904223u; r.ymx.l[k] = x >> 4; x = x * 1664525u + 1013904223u; r.ypx.l[k] = x >> 4; x = x * 1664525u + 1013904223u; r.td.l[k] = x >> 4; }
    r.ymx.l[13] &= 0xffff; r.ypx.l[13] &= 0xffff; r.td.l[13] &= 0xffff;
    for (int k = 0; k < 6; k++) r.pad[k] = 0;
    tab[i] = r;
}

#include "capi_common.hpp"
extern "C" const char *zkaes_last_error(void);
namespace zk { void capi_set_error(const std::string &); }

namespace {
template <class Fn> int guardk(Fn &&fn) {
    try { zk::capi_set_error(""); fn(); return 0; }
    catch (const std::exception &e) { zk::capi_set_error(e.what()); return 1; }
    catch (...) { zk::capi_set_error("unknown error"); return 1; }
}
using zk::gpu::DevPtr; using zk::gpu::StreamGuard; using zk::gpu::WorkspaceGuard; using zk::gpu::EventGuard;
// Every helper below validates its arguments BEFORE it allocates and owns its temporaries through RAII guards (gpu.hpp): a GpuError in the middle of a call -- a bad coset
// index, an MSM whose n x windows exceeds the sort's 2^31 pairs, a device fault -- releases the stream, the buffers and the MSM workspace on the way out
// (tests/test_gpu_kernels.py::test_error_paths_release_device_memory).
int exact_log2(size_t n, const char *who) {
    int lg = 0;
    while (((size_t)1 << lg) < n) lg++;
    if (n == 0 || ((size_t)1 << lg) != n) throw std::invalid_argument(std::string(who) + ": n must be a power of two");
    return lg;
}
template <class Fr> void run_ntt(uint8_t *data, size_t n, int inverse, int coset_c, int lg_big) {
    const int lg = exact_log2(n, "zkaes_ntt");
    if (!data) throw std::invalid_argument("zkaes_ntt: null data");
    zk::gpu::require_device();
    StreamGuard s;
    DevPtr<Fr> a(n), b(n);
    zk::gpu::h2d(a, data, n * sizeof(Fr), s);
    if (coset_c) zk::gpu::ntt_coset<Fr>(b, a, n, lg, inverse != 0, coset_c, lg_big, s);
    else zk::gpu::ntt<Fr>(b, a, n, lg, inverse != 0, s);
    zk::gpu::d2h(data, b, n * sizeof(Fr), s);
}
template <class Fr> void run_ntt_batch(uint8_t *data, size_t n, int count, int inverse, const int *coset_c, int lg_big) {
    const int lg = exact_log2(n, "zkaes_ntt_batch");
    if (count < 1 || count > 12) throw std::invalid_argument("zkaes_ntt_batch: 1..12 transforms");
    if (!data) throw std::invalid_argument("zkaes_ntt_batch: null data");
    zk::gpu::require_device();
    StreamGuard s;
    DevPtr<Fr> a((size_t)count * n), b((size_t)count * n);
    zk::gpu::h2d(a, data, (size_t)count * n * sizeof(Fr), s);
    zk::gpu::NttJob<Fr> jobs[12];
    for (int i = 0; i < count; i++) jobs[i] = zk::gpu::NttJob<Fr>{b + (size_t)i * n, a + (size_t)i * n, coset_c ? coset_c[i] : 0};
    zk::gpu::ntt_batch<Fr>(jobs, count, n, lg, inverse != 0, lg_big, s);
    zk::gpu::d2h(data, b, (size_t)count * n * sizeof(Fr), s);
}
template <class Fq> void give_affine(const zk::Affine<Fq> &a, uint8_t *out_xy, int *out_inf) {
    if (out_inf) *out_inf = a.is_inf() ? 1 : 0;
    if (out_xy) { memcpy(out_xy, a.x.l, 48); memcpy(out_xy + 48, a.y.l, 48); }
}
template <class Curve> void run_msm(const uint8_t *bases, const uint8_t *scalars, size_t n, uint8_t *out_xy, int *out_inf, int reps, double *ms_total, double *ms_acc) {
    using Fq = typename Curve::Fq; using Fr = typename Curve::Fr;
    if (n && (!bases || !scalars)) throw std::invalid_argument("zkaes_msm: null argument");
    if (n >= ((size_t)1 << 30)) throw std::invalid_argument("zkaes_msm: too many points");
    zk::gpu::require_device();
    StreamGuard s;
    DevPtr<zk::Affine<Fq>> db(n);
    DevPtr<Fr> ds(n);
    zk::gpu::h2d(db, bases, n * 96, s); zk::gpu::h2d(ds, scalars, n * 32, s);
    DevPtr<zk::Affine28<typename Curve::FqP>> db28(n);
    zk::gpu::convert_bases<Curve>(db28, db, n, s);
    zk::gpu::sync(s);
    WorkspaceGuard ws;
    zk::XYZZ<Fq> r = zk::gpu::msm<Curve>(ws, db28, ds, n, s);   // warm-up / result
    if (reps > 0) {
        zk::gpu::MsmStats before = zk::gpu::msm_stats(false);
        EventGuard e0, e1;
        zk::gpu::event_record(e0, s);
        for (int i = 0; i < reps; i++) r = zk::gpu::msm<Curve>(ws, db28, ds, n, s);
        zk::gpu::event_record(e1, s);
        float ms = zk::gpu::event_elapsed_ms(e0, e1);
        zk::gpu::MsmStats after = zk::gpu::msm_stats(false);
        if (ms_total) *ms_total = ms / reps;
        if (ms_acc) *ms_acc = (after.accumulate_ms - before.accumulate_ms) / reps;
    }
    give_affine(r.to_affine(), out_xy, out_inf);
}
// EDWARDS (377 only): the prover's SRS path -- tables on the curve's twisted Edwards model; the bases must lie in the prime-order subgroup.  Otherwise the
// Weierstrass law (any curve point).
template <class Curve, bool EDWARDS> void run_msm_table(const uint8_t *bases, const uint8_t *scalars, size_t n, int c, uint8_t *out_xy, int *out_inf) {
    using Fq = typename Curve::Fq; using Fr = typename Curve::Fr;
    if (c < 2 || c > 22) throw std::invalid_argument("window bits must be in [2, 22]");
    if (n && (!bases || !scalars)) throw std::invalid_argument("zkaes_msm_table: null argument");
    zk::gpu::require_device();
    const size_t nt = (size_t)zk::gpu::table_windows<Curve>(c);
    if ((uint64_t)nt * n >= (1ull << 30)) throw std::invalid_argument("zkaes_msm_table: n x table copies exceeds the 2^30 base indices of one MSM");
    StreamGuard s;
    DevPtr<zk::Affine<Fq>> tab(nt * n);
    DevPtr<Fr> ds(n);
    zk::gpu::h2d(tab, bases, n * 96, s); zk::gpu::h2d(ds, scalars, n * 32, s);
    zk::gpu::build_window_tables<Curve>(tab, n, c, s);
    WorkspaceGuard ws;
    zk::Affine<Fq> a;
    if constexpr (EDWARDS) {
        DevPtr<zk::Niels28<typename Curve::FqP>> tabte(nt * n);
        zk::gpu::convert_bases_te<Curve>(tabte, tab, nt * n, s);
        a = zk::gpu::msm_table<Curve>(ws, tabte, n, 0, c, ds, n, s).to_affine();
    } else {
        DevPtr<zk::Affine28<typename Curve::FqP>> tab28(nt * n);
        zk::gpu::convert_bases<Curve>(tab28, tab, nt * n, s);
        a = zk::gpu::msm_table<Curve>(ws, tab28, n, 0, c, ds, n, s).to_affine();
    }
    give_affine(a, out_xy, out_inf);
}
template <class Curve> void run_msm_window_sums_dev(const uint8_t *bases, const uint8_t *scalars, size_t n_local, size_t n_total, void *dev_out, size_t dev_out_bytes) {
    using Fq = typename Curve::Fq; using Fr = typename Curve::Fr;
    zk::gpu::require_device();
    int c = 0, nwin = 0;
    zk::gpu::msm_sharded_plan<Curve>(n_total, &c, &nwin);
    if (!dev_out || dev_out_bytes < (size_t)nwin * sizeof(zk::XYZZ<Fq>)) throw std::invalid_argument("zkaes_msm_window_sums_dev: device buffer too small for the window sums");
    if (n_local > n_total) throw std::invalid_argument("zkaes_msm_window_sums_dev: n_local > n_total");
    if (n_local && (!bases || !scalars)) throw std::invalid_argument("zkaes_msm_window_sums_dev: null argument");
    StreamGuard s;
    DevPtr<zk::Affine<Fq>> db(n_local);
    DevPtr<Fr> ds(n_local);
    zk::gpu::h2d(db, bases, n_local * 96, s); zk::gpu::h2d(ds, scalars, n_local * 32, s);
    DevPtr<zk::Affine28<typename Curve::FqP>> db28(n_local);
    zk::gpu::convert_bases<Curve>(db28, db, n_local, s);
    WorkspaceGuard ws;
    zk::gpu::msm_window_sums_device<Curve>(ws, db28, ds, n_local, n_total, (zk::XYZZ<Fq> *)dev_out, s);    // synchronizes the stream
}
constexpr int MAX_FOLD_WORLD = 4096;        // ranks whose partial sums one fold call adds (an 8-GPU node needs 8)
template <class Curve> void run_msm_fold_dev(const void *dev_in, int world, size_t n_total, uint8_t *out_xy, int *out_inf) {
    using Fq = typename Curve::Fq;
    if (!dev_in || world < 1 || world > MAX_FOLD_WORLD) throw std::invalid_argument("zkaes_msm_fold_window_sums_dev: bad arguments (world must be 1..4096)");
    zk::gpu::require_device();
    StreamGuard s;
    give_affine(zk::gpu::msm_fold_window_sums_device<Curve>((const zk::XYZZ<Fq> *)dev_in, world, n_total, s).to_affine(), out_xy, out_inf);
}
// host-side sum of a handful of affine partial results: the "local EC add" after the all-gather of a point-range-sharded MSM
template <class Curve> void run_g1_sum(const uint8_t *points_xy, const int *inf, size_t n, uint8_t *out_xy, int *out_inf) {
    using Fq = typename Curve::Fq;
    zk::XYZZ<Fq> acc = zk::XYZZ<Fq>::inf();
    for (size_t i = 0; i < n; i++) {
        if (inf && inf[i]) continue;
        zk::Affine<Fq> a;
        memcpy(a.x.l, points_xy + 96 * i, 48); memcpy(a.y.l, points_xy + 96 * i + 48, 48);
        acc.add(zk::XYZZ<Fq>::from_affine(a));
    }
    zk::Affine<Fq> r = acc.to_affine();
    *out_inf = r.is_inf() ? 1 : 0;
    memcpy(out_xy, r.x.l, 48); memcpy(out_xy + 48, r.y.l, 48);
}

// ---- the prover's polynomial kernels (kernels_poly.hip) and the NTT entry points the prover uses but zkaes_ntt does not reach, one launch wrapper per call: host byte
// buffers of 32-byte Montgomery limbs in and out, so that a test can compare every multi-launch algorithm with a big-integer model at the block, chunk and level
// boundaries of its constants (tests/test_gpu_poly.py).  Elements must be canonical (< r); they are not checked one by one.
using PF = zk::gpu::F;
PF load_f(const uint8_t *b, const char *who) {
    if (!b) throw std::invalid_argument(std::string(who) + ": null field element");
    PF x; memcpy(x.l, b, 32); return x;
}
void need(bool ok, const char *who, const char *what) { if (!ok) throw std::invalid_argument(std::string(who) + ": " + what); }
constexpr size_t POLY_MAX = (size_t)1 << 28;        // elements per array a kernel-level call accepts (8 GB)
// device copy of `count` host elements (at least one element is allocated, so that the pointer is valid for an empty array)
DevPtr<PF> upload(const uint8_t *host, size_t count, zk::gpu::stream_t s) {
    DevPtr<PF> d(count ? count : 1);
    zk::gpu::h2d(d, host, count * sizeof(PF), s);
    return d;
}
template <class Fr> void run_ntt_padded(const uint8_t *in, size_t in_len, size_t n, int inverse, int coset_c, int lg_big, uint8_t *out) {
    const int lg = exact_log2(n, "zkaes_ntt_padded");
    need(in_len <= n, "zkaes_ntt_padded", "in_len must not exceed n");
    need(out && (in || !in_len), "zkaes_ntt_padded", "null argument");
    need(coset_c >= 0, "zkaes_ntt_padded", "coset index must not be negative");
    zk::gpu::require_device();
    StreamGuard s;
    DevPtr<Fr> a(in_len ? in_len : 1), b(n);
    zk::gpu::h2d(a, in, in_len * sizeof(Fr), s);
    if (coset_c) zk::gpu::ntt_coset<Fr>(b, a, in_len, lg, inverse != 0, coset_c, lg_big, s);
    else zk::gpu::ntt<Fr>(b, a, in_len, lg, inverse != 0, s);
    zk::gpu::d2h(out, b, n * sizeof(Fr), s);
}

// ---- the MSM forms the PROVER calls (marlin.cpp), which zkaes_msm / zkaes_msm_table do not reach: class sums, two scalar vectors in one Pippenger instance, one prepared
// state against two base arrays, and table mode over a sub-range of a longer table.  BLS12-377; EDWARDS selects the prover's law (Niels28 records on the twisted Edwards
// model), otherwise Affine28 bases on the Weierstrass model.  Standard affine bases and Montgomery scalars in, as zkaes_msm takes them (tests/test_gpu_msm_forms.py).
using MC = zk::Bls377;
using MFq = zk::Fq377;
using MFr = zk::Fr377;
using MP = zk::Fq377P;
constexpr size_t MSM_FORM_MAX = (size_t)1 << 26;       // bases per call (6 GB of standard affine points)
template <bool EDWARDS> using MsmBase = typename std::conditional<EDWARDS, zk::Niels28<MP>, zk::Affine28<MP>>::type;
template <bool EDWARDS> DevPtr<MsmBase<EDWARDS>> law_bases(const zk::Affine<MFq> *src, size_t n, zk::gpu::stream_t s) {
    DevPtr<MsmBase<EDWARDS>> d(n ? n : 1);
    if constexpr (EDWARDS) zk::gpu::convert_bases_te<MC>(d, src, n, s); else zk::gpu::convert_bases<MC>(d, src, n, s);
    zk::gpu::sync(s);        // the caller may release `src` at once
    return d;
}
DevPtr<zk::Affine<MFq>> upload_points(const uint8_t *host, size_t count, size_t room, zk::gpu::stream_t s) {
    DevPtr<zk::Affine<MFq>> d(room ? room : 1);
    zk::gpu::h2d(d, host, count * 96, s);
    return d;
}
DevPtr<MFr> upload_scalars(const uint8_t *host, size_t count, zk::gpu::stream_t s) {
    DevPtr<MFr> d(count ? count : 1);
    zk::gpu::h2d(d, host, count * 32, s);
    return d;
}
void check_table_bits(int c, size_t stride, const char *who) {
    if (c < 2 || c > 22) throw std::invalid_argument("window bits must be in [2, 22]");
    need((uint64_t)zk::gpu::table_windows<MC>(c) * stride < (1ull << 30), who, "stride x table copies exceeds the 2^30 base indices of one MSM");
}
template <bool EDWARDS>
void run_class_sum(const uint8_t *bases, size_t n, const int8_t *vals, int count, size_t prior, int *ok_out, uint8_t *out_xy, int *out_inf) {
    zk::gpu::require_device();
    StreamGuard s;
    DevPtr<zk::Affine<MFq>> db = upload_points(bases, n, n, s);
    DevPtr<MsmBase<EDWARDS>> dl = law_bases<EDWARDS>(db, n, s);
    db.reset();              // (a million points: give the standard-form copy back before the class sums grow their scratch)
    DevPtr<int8_t> dv((size_t)count * n);
    zk::gpu::h2d(dv, vals, (size_t)count * n, s);
    WorkspaceGuard ws;
    if (prior) {       // a generic MSM first: the class sums then carve their scratch from a bucket array that MSM sized (a prover context's second proof)
        std::vector<MFr> sc(prior);
        uint64_t x = 88172645463325252ull;
        for (size_t i = 0; i < prior; i++) { for (int k = 0; k < 8; k += 2) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; sc[i].l[k] = (uint32_t)x; sc[i].l[k + 1] = (uint32_t)(x >> 32); } sc[i].l[7] &= 0x0fffffffu; }
        DevPtr<MFr> ds = upload_scalars((const uint8_t *)sc.data(), prior, s);
        zk::gpu::sync(s);
        (void)zk::gpu::msm<MC>(ws, (const MsmBase<EDWARDS> *)dl.get(), (const MFr *)ds.get(), prior, s);
    }
    for (int v = 0; v < count; v++) {
        zk::XYZZ<MFq> r;
        const bool ok = zk::gpu::class_sum<MC>(ws, (const MsmBase<EDWARDS> *)dl.get(), (const int8_t *)dv.get() + (size_t)v * n, n, &r, s);
        ok_out[v] = ok ? 1 : 0;
        if (ok) give_affine(r.to_affine(), out_xy + 96 * (size_t)v, out_inf + v);
        else { memset(out_xy + 96 * (size_t)v, 0, 96); out_inf[v] = 0; }
    }
}
template <bool EDWARDS>
void run_msm_pair(const uint8_t *bases, size_t nbases, const uint8_t *scal1, size_t n1, const uint8_t *scal2, size_t n2, size_t val_off2, uint8_t *out_xy, int *out_inf) {
    zk::gpu::require_device();
    StreamGuard s;
    DevPtr<zk::Affine<MFq>> db = upload_points(bases, nbases, nbases, s);
    DevPtr<MsmBase<EDWARDS>> dl = law_bases<EDWARDS>(db, nbases, s);
    DevPtr<MFr> d1 = upload_scalars(scal1, n1, s), d2 = upload_scalars(scal2, n2, s);
    zk::gpu::sync(s);
    WorkspaceGuard ws;
    zk::gpu::msm_prepare<MC>(ws, d1, n1, n2 ? d2.get() : nullptr, n2, n2 ? val_off2 : 0, s);
    give_affine(zk::gpu::msm_finish<MC>(ws, (const MsmBase<EDWARDS> *)dl.get(), s).to_affine(), out_xy, out_inf);
}
// window tables over all `stride` bases in the law's form: copy j at j * stride
template <bool EDWARDS> DevPtr<MsmBase<EDWARDS>> law_tables(const uint8_t *bases, size_t stride, int c, zk::gpu::stream_t s) {
    const size_t nt = (size_t)zk::gpu::table_windows<MC>(c);
    DevPtr<zk::Affine<MFq>> tab = upload_points(bases, stride, nt * stride, s);
    zk::gpu::build_window_tables<MC>(tab, stride, c, s);
    return law_bases<EDWARDS>(tab, nt * stride, s);
}
template <bool EDWARDS>
void run_msm_table_pair(const uint8_t *bases, size_t stride, const uint8_t *scal1, size_t n1, size_t off1, const uint8_t *scal2, size_t n2, size_t off2, int c, uint8_t *out_xy, int *out_inf) {
    zk::gpu::require_device();
    StreamGuard s;
    DevPtr<MsmBase<EDWARDS>> tabs = law_tables<EDWARDS>(bases, stride, c, s);
    DevPtr<MFr> d1 = upload_scalars(scal1, n1, s), d2 = upload_scalars(scal2, n2, s);
    zk::gpu::sync(s);
    WorkspaceGuard ws;
    zk::gpu::msm_prepare_table<MC>(ws, d1, n1, off1, n2 ? d2.get() : nullptr, n2, n2 ? off2 : 0, c, stride, s);
    give_affine(zk::gpu::msm_finish<MC>(ws, (const MsmBase<EDWARDS> *)tabs.get(), s).to_affine(), out_xy, out_inf);
}
void run_msm_second_bases(const uint8_t *bases, size_t nbases, const uint8_t *scalars, size_t n, size_t off, size_t shift, int c, uint8_t *out_xy, int *out_inf) {
    zk::gpu::require_device();
    StreamGuard s;
    DevPtr<MFr> ds = upload_scalars(scalars, n, s);
    WorkspaceGuard ws;
    zk::XYZZ<MFq> r[2];
    if (c == 0) {
        DevPtr<zk::Affine<MFq>> db = upload_points(bases, nbases, nbases, s);
        DevPtr<zk::Niels28<MP>> dl = law_bases<true>(db, nbases, s);
        zk::gpu::msm_prepare<MC>(ws, ds, n, nullptr, 0, 0, s);
        zk::gpu::msm_finish2<MC>(ws, dl.get() + off, dl.get() + off + shift, r, s);
    } else {
        DevPtr<zk::Niels28<MP>> tabs = law_tables<true>(bases, nbases, c, s);
        zk::gpu::msm_prepare_table<MC>(ws, ds, n, off, nullptr, 0, 0, c, nbases, s);
        zk::gpu::msm_finish2<MC>(ws, tabs.get(), tabs.get() + shift, r, s);
    }
    for (int i = 0; i < 2; i++) give_affine(r[i].to_affine(), out_xy + 96 * i, out_inf + i);
}

// ---- the same forms as a SEQUENCE on one workspace and one stream (include/zkaes.h zkaes_msm_sequence; tests/test_gpu_msm_workspace.py): what a prover context and the batch
// verifier do with theirs, and what every runner above, with a workspace of its own per call, cannot show.
constexpr size_t MSM_SEQ_MAX_TABLES = 8;              // distinct window bits per law and call
// the bases in one law's forms: the plain records, and window tables of stride nbases per distinct window bits
template <bool EDWARDS> struct SeqForms {
    DevPtr<MsmBase<EDWARDS>> plain;
    std::vector<std::pair<int, DevPtr<MsmBase<EDWARDS>>>> tables;
    bool want_plain = false;
    std::vector<int> want_bits;
    void want(int c) {
        if (!c) want_plain = true;
        else if (std::find(want_bits.begin(), want_bits.end(), c) == want_bits.end()) want_bits.push_back(c);
    }
    void build(const uint8_t *bases, size_t nbases, zk::gpu::stream_t s) {
        if (want_plain) {
            DevPtr<zk::Affine<MFq>> db = upload_points(bases, nbases, nbases, s);
            plain = law_bases<EDWARDS>(db, nbases, s);
        }
        for (int c : want_bits) tables.emplace_back(c, law_tables<EDWARDS>(bases, nbases, c, s));
    }
    const MsmBase<EDWARDS> *get(int c) const {
        if (!c) return plain.get();
        for (auto &t : tables) if (t.first == c) return t.second.get();
        return nullptr;
    }
};
struct SeqBases {
    SeqForms<true> te;
    SeqForms<false> we;
    void want(bool edwards, int c) { if (edwards) te.want(c); else we.want(c); }
    // msm_finish over the form (law, c), every base index moved up by `at`
    zk::XYZZ<MFq> finish(zk::gpu::MsmWorkspace *ws, bool edwards, int c, size_t at, zk::gpu::stream_t s) const {
        if (edwards) { const zk::Niels28<MP> *b = te.get(c); need(b != nullptr, "zkaes_msm_sequence", "no base form for this step"); return zk::gpu::msm_finish<MC>(ws, b + at, s); }
        const zk::Affine28<MP> *b = we.get(c);
        need(b != nullptr, "zkaes_msm_sequence", "no base form for this step");
        return zk::gpu::msm_finish<MC>(ws, b + at, s);
    }
};
// what the last preparing step left in the workspace: window bits (0: per-window), the index its base pointer started at, one past the highest index it names from there
struct SeqPrepared { bool live = false; int c = 0; size_t origin = 0, extent = 0; };
bool seq_prepares(uint32_t kind) { return kind == ZKAES_STEP_WINDOW || kind == ZKAES_STEP_TABLE || kind == ZKAES_STEP_SECOND; }
// everything that can be judged without the device, before anything is allocated; leaves the forms the steps need in `forms`
void check_msm_sequence(const zkaes_msm_step *steps, size_t nsteps, size_t nbases, size_t nscalars, size_t nvals, SeqBases &forms) {
    const char *who = "zkaes_msm_sequence";
    int prepared_c = -1;
    for (size_t i = 0; i < nsteps; i++) {
        const zkaes_msm_step &st = steps[i];
        need(st.kind <= ZKAES_STEP_REFINISH && st.reserved == 0, who, "unknown step kind");
        need(st.off1 <= MSM_FORM_MAX && st.off2 <= MSM_FORM_MAX && st.shift <= MSM_FORM_MAX && st.n1 <= MSM_FORM_MAX && st.n2 <= MSM_FORM_MAX, who, "step lengths and offsets must not exceed 2^26");
        const bool edwards = st.edwards != 0;
        const int c = (int)st.window_bits;
        if (st.kind == ZKAES_STEP_CLASS) {
            need(st.scal1 <= nvals && st.n1 <= nvals - st.scal1, who, "value range outside the class values");
            forms.want(edwards, 0);
        } else if (st.kind == ZKAES_STEP_REFINISH) {
            need(prepared_c >= 0, who, "a refinish step needs a preparing step before it");
            forms.want(edwards, prepared_c);
        } else {
            need(st.scal1 <= nscalars && st.n1 <= nscalars - st.scal1, who, "scalar range outside the scalars");
            const bool pair = st.kind != ZKAES_STEP_SECOND && st.n2;
            need(!pair || (st.scal2 <= nscalars && st.n2 <= nscalars - st.scal2), who, "scalar range outside the scalars");
            need(st.kind != ZKAES_STEP_SECOND || edwards, who, "two base arrays per prepared state need the Edwards law");
            const bool table = st.kind == ZKAES_STEP_TABLE || (st.kind == ZKAES_STEP_SECOND && c != 0);
            if (table) check_table_bits(c, nbases, who);
            prepared_c = table ? c : 0;
            forms.want(edwards, prepared_c);
        }
    }
    need(forms.te.want_bits.size() <= MSM_SEQ_MAX_TABLES && forms.we.want_bits.size() <= MSM_SEQ_MAX_TABLES, who, "at most 8 distinct window bits per law");
}
void run_msm_sequence(const uint8_t *bases, size_t nbases, const uint8_t *scalars, size_t nscalars, const int8_t *vals, size_t nvals, const zkaes_msm_step *steps, size_t nsteps, bool poison,
                      SeqBases &forms, uint8_t *out_xy, int *out_inf, int *out_ok, int *out_status, char *out_err) {
    const char *who = "zkaes_msm_sequence";
    zk::gpu::require_device();
    StreamGuard s;
    forms.te.build(bases, nbases, s);
    forms.we.build(bases, nbases, s);
    DevPtr<MFr> ds = upload_scalars(scalars, nscalars, s);
    DevPtr<int8_t> dv(nvals ? nvals : 1);
    zk::gpu::h2d(dv, vals, nvals, s);
    zk::gpu::sync(s);
    WorkspaceGuard ws;                   // ONE workspace for every step: nothing below may make another
    SeqPrepared prep;
    for (size_t i = 0; i < nsteps; i++) {
        const zkaes_msm_step &st = steps[i];
        uint8_t *xy = out_xy + 192 * i;
        int *inf = out_inf + 2 * i;
        memset(xy, 0, 192); inf[0] = inf[1] = 0; out_ok[i] = 0; out_status[i] = 0; out_err[ZKAES_MSM_SEQ_ERR_BYTES * i] = 0;
        const bool edwards = st.edwards != 0;
        const int c = (int)st.window_bits;
        const SeqPrepared before = prep;
        prep.live = false;               // (set again by a step that leaves a prepared state behind)
        try {
            if (poison && i) zk::gpu::msm_workspace_poison_accumulators(ws, s);
            const MFr *s1 = seq_prepares(st.kind) ? ds.get() + st.scal1 : nullptr, *s2 = s1 && st.kind != ZKAES_STEP_SECOND && st.n2 ? ds.get() + st.scal2 : nullptr;
            if (st.kind == ZKAES_STEP_WINDOW) {
                const size_t off2 = st.n2 ? st.off2 : 0;
                need(st.off1 <= nbases && st.n1 <= nbases - st.off1 && off2 <= nbases - st.off1 && st.n2 <= nbases - st.off1 - off2, who, "range exceeds the bases");
                zk::gpu::msm_prepare<MC>(ws, s1, st.n1, s2, st.n2, off2, s);
                give_affine(forms.finish(ws, edwards, 0, st.off1, s).to_affine(), xy, inf);
                prep = SeqPrepared{true, 0, (size_t)st.off1, std::max((size_t)st.n1, (size_t)(off2 + st.n2))};
            } else if (st.kind == ZKAES_STEP_TABLE) {       // (its ranges are msm_prepare_table's to judge: "msm_table: range exceeds the table")
                zk::gpu::msm_prepare_table<MC>(ws, s1, st.n1, st.off1, s2, st.n2, st.n2 ? st.off2 : 0, c, nbases, s);
                give_affine(forms.finish(ws, edwards, c, 0, s).to_affine(), xy, inf);
                prep = SeqPrepared{true, c, 0, std::max((size_t)(st.n1 ? st.off1 + st.n1 : 0), (size_t)(st.n2 ? st.off2 + st.n2 : 0))};
            } else if (st.kind == ZKAES_STEP_SECOND) {
                const zk::Niels28<MP> *b = forms.te.get(c);
                need(b != nullptr, who, "no base form for this step");
                if (st.off1 > nbases || st.shift > nbases - st.off1 || st.n1 > nbases - st.off1 - st.shift)
                    throw std::invalid_argument(c ? "msm_table: range exceeds the table" : "zkaes_msm_sequence: range exceeds the bases");
                zk::XYZZ<MFq> r[2];
                if (c == 0) {
                    zk::gpu::msm_prepare<MC>(ws, s1, st.n1, nullptr, 0, 0, s);
                    zk::gpu::msm_finish2<MC>(ws, b + st.off1, b + st.off1 + st.shift, r, s);
                    prep = SeqPrepared{true, 0, (size_t)st.off1, (size_t)st.n1};
                } else {
                    zk::gpu::msm_prepare_table<MC>(ws, s1, st.n1, st.off1, nullptr, 0, 0, c, nbases, s);
                    zk::gpu::msm_finish2<MC>(ws, b, b + st.shift, r, s);
                    prep = SeqPrepared{true, c, 0, (size_t)(st.n1 ? st.off1 + st.n1 : 0)};
                }
                for (int k = 0; k < 2; k++) give_affine(r[k].to_affine(), xy + 96 * k, inf + k);
            } else if (st.kind == ZKAES_STEP_CLASS) {
                need(st.off1 <= nbases && st.n1 <= nbases - st.off1, who, "range exceeds the bases");
                zk::XYZZ<MFq> r;
                const int8_t *v = dv.get() + st.scal1;
                const bool ok = edwards ? zk::gpu::class_sum<MC>(ws, forms.te.get(0) + st.off1, v, st.n1, &r, s) : zk::gpu::class_sum<MC>(ws, forms.we.get(0) + st.off1, v, st.n1, &r, s);
                if (ok) give_affine(r.to_affine(), xy, inf);
                out_ok[i] = ok ? 1 : 0;
                continue;
            } else {                                        // ZKAES_STEP_REFINISH
                need(before.live, who, "no prepared state to finish again: the step before prepared none");
                need(before.origin + before.extent + st.shift <= nbases, who, "range exceeds the bases");
                give_affine(forms.finish(ws, edwards, before.c, before.origin + st.shift, s).to_affine(), xy, inf);
                prep = before;
            }
            out_ok[i] = 1;
        } catch (const std::exception &e) {
            // a refusal is recorded and the sequence goes on; after an error of the device itself nothing more is launched
            if (!strncmp(e.what(), "HIP error", 9)) throw;
            prep.live = false;
            memset(xy, 0, 192); inf[0] = inf[1] = 0;
            out_status[i] = 1;
            snprintf(out_err + ZKAES_MSM_SEQ_ERR_BYTES * i, ZKAES_MSM_SEQ_ERR_BYTES, "%s", e.what());
        }
    }
}

// ---- the prover's R1CS and randomness kernels (kernels_witness.hip, kernels_poly.hip), which run only inside whole proofs otherwise (tests/test_gpu_r1cs.py).  Every
// output and scratch buffer is filled with 0xAB bytes on the device before the call, so that a slot a kernel fails to write shows up as a mismatch.
template <class T> DevPtr<T> poisoned(size_t count, zk::gpu::stream_t s) {
    DevPtr<T> d(count ? count : 1);
    HIP_CHECK(hipMemsetAsync(d.get(), 0xAB, (count ? count : 1) * zk::gpu::DevElem<T>::bytes, (hipStream_t)s));
    return d;
}
template <class T> DevPtr<T> upload_as(const T *host, size_t count, zk::gpu::stream_t s) {
    DevPtr<T> d(count ? count : 1);
    zk::gpu::h2d(d, host, count * sizeof(T), s);
    return d;
}
constexpr size_t R1CS_MAX = (size_t)1 << 24;           // rows, columns, entries and elements a kernel-level R1CS call accepts
// a CSR triple as the caller states it: rowptr[0] = 0, rowptr non-decreasing over rows + 1 entries, every column below ncols; returns the entry count
size_t check_csr(const uint32_t *rowptr, const uint32_t *col, const int64_t *coeff, size_t rows, size_t ncols, const char *who) {
    need(rowptr != nullptr, who, "null rowptr");
    need(rowptr[0] == 0, who, "rowptr must start at 0");
    for (size_t r = 0; r < rows; r++) need(rowptr[r] <= rowptr[r + 1], who, "rowptr must not decrease");
    const size_t nnz = rowptr[rows];
    need(nnz <= R1CS_MAX, who, "too many entries");
    need(!nnz || (col && coeff), who, "null entries");
    for (size_t i = 0; i < nnz; i++) need(col[i] < ncols, who, "column index out of range");
    return nnz;
}
bool is_pow2(size_t n) { return n && !(n & (n - 1)); }

// ---- the kernels that build a key (kernels_msm.hip k_power_scalars, k_fixed_base, k_table_next, k_convert_bases_te; kernels_poly.hip k_index_rowcol, k_index_vals), which
// otherwise run once per SRS or per key inside key synthesis (tests/test_gpu_keysynth.py).  Points cross as 96-byte standard affine x || y, infinity as 96 zero bytes --
// the library's own encoding, copied as it is.  Every output buffer is poisoned first.
constexpr size_t KEYSYNTH_MAX = (size_t)1 << 20;       // points or elements a kernel-level key-synthesis call accepts
template <class Fq> zk::Affine<Fq> load_point(const uint8_t *xy) { zk::Affine<Fq> a; memcpy(a.x.l, xy, 48); memcpy(a.y.l, xy + 48, 48); return a; }
template <class Curve> void run_fixed_base_powers(const uint8_t *base_xy, const uint8_t *beta, uint64_t from, size_t count, size_t chunk, uint8_t *out) {
    using Fq = typename Curve::Fq; using Fr = typename Curve::Fr;
    Fr b; memcpy(b.l, beta, 32);
    zk::gpu::require_device();
    StreamGuard s;
    DevPtr<zk::Affine<Fq>> d = poisoned<zk::Affine<Fq>>(count, s);
    zk::gpu::fixed_base_powers<Curve>(d, load_point<Fq>(base_xy), b, (size_t)from, count, s, chunk);
    zk::gpu::d2h(out, d, count * 96, s);
}
template <class Curve> void run_table_next(const uint8_t *prev, size_t count, int c, int j, uint8_t *out) {
    using Fq = typename Curve::Fq;
    zk::gpu::require_device();
    StreamGuard s;
    DevPtr<zk::Affine<Fq>> dp(count), dn = poisoned<zk::Affine<Fq>>(count, s);
    zk::gpu::h2d(dp, prev, count * 96, s);
    zk::gpu::table_next<Curve>(dn, dp, count, c, j, s);
    zk::gpu::d2h(out, dn, count * 96, s);
}
template <class Curve> void run_build_window_tables(const uint8_t *bases, size_t n, int c, uint8_t *out) {
    using Fq = typename Curve::Fq;
    zk::gpu::require_device();
    const size_t nt = (size_t)zk::gpu::table_windows<Curve>(c);
    StreamGuard s;
    DevPtr<zk::Affine<Fq>> tab = poisoned<zk::Affine<Fq>>(nt * n, s);
    zk::gpu::h2d(tab, bases, n * 96, s);
    zk::gpu::build_window_tables<Curve>(tab, n, c, s);
    zk::gpu::d2h(out, tab, nt * n * 96, s);
}
void check_curve_table_args(int curve_id, int c, size_t count, const char *who) {
    need(curve_id == 377 || curve_id == 381, who, "curve_id must be 377 or 381");
    if (c < 2 || c > 22) throw std::invalid_argument("window bits must be in [2, 22]");
    need(count >= 1 && count <= KEYSYNTH_MAX, who, "count out of range");
}
}  // namespace

extern "C" {
// ---- kernel-level entry points of the MSM forms the prover calls (include/zkaes.h): every argument is checked before anything is allocated
int zkaes_class_sum(const uint8_t *bases, size_t n, const int8_t *vals, int count, int edwards, size_t prior_msm_points, int *ok_out, uint8_t *out_xy, int *out_inf) {
    return guardk([&] {
        const char *who = "zkaes_class_sum";
        need(count >= 1 && count <= 8, who, "1..8 value vectors");
        need(bases && vals && ok_out && out_xy && out_inf, who, "null argument");
        need(n >= 1 && n <= MSM_FORM_MAX, who, "n out of range");
        need(prior_msm_points <= n, who, "the prior MSM runs over the same bases: at most n points");
        if (edwards) run_class_sum<true>(bases, n, vals, count, prior_msm_points, ok_out, out_xy, out_inf);
        else run_class_sum<false>(bases, n, vals, count, prior_msm_points, ok_out, out_xy, out_inf);
    });
}
int zkaes_msm_pair(const uint8_t *bases, size_t nbases, const uint8_t *scal1, size_t n1, const uint8_t *scal2, size_t n2, size_t val_off2, int edwards, uint8_t *out_xy, int *out_inf) {
    return guardk([&] {
        const char *who = "zkaes_msm_pair";
        need(out_xy && out_inf && (bases || !nbases) && (scal1 || !n1) && (scal2 || !n2), who, "null argument");
        need(nbases <= MSM_FORM_MAX, who, "too many bases");
        need(n1 <= nbases && val_off2 <= nbases && n2 <= nbases - val_off2, who, "range exceeds the bases");
        if (edwards) run_msm_pair<true>(bases, nbases, scal1, n1, scal2, n2, val_off2, out_xy, out_inf);
        else run_msm_pair<false>(bases, nbases, scal1, n1, scal2, n2, val_off2, out_xy, out_inf);
    });
}
int zkaes_msm_table_pair(const uint8_t *bases, size_t stride, const uint8_t *scal1, size_t n1, size_t off1, const uint8_t *scal2, size_t n2, size_t off2, int window_bits, int edwards,
                         uint8_t *out_xy, int *out_inf) {
    return guardk([&] {
        const char *who = "zkaes_msm_table_pair";
        need(out_xy && out_inf && (bases || !stride) && (scal1 || !n1) && (scal2 || !n2), who, "null argument");
        need(stride <= MSM_FORM_MAX, who, "too many bases");
        check_table_bits(window_bits, stride, who);
        if (off1 > stride || n1 > stride - off1 || off2 > stride || n2 > stride - off2) throw std::invalid_argument("msm_table: range exceeds the table");
        if (edwards) run_msm_table_pair<true>(bases, stride, scal1, n1, off1, scal2, n2, off2, window_bits, out_xy, out_inf);
        else run_msm_table_pair<false>(bases, stride, scal1, n1, off1, scal2, n2, off2, window_bits, out_xy, out_inf);
    });
}
int zkaes_msm_second_bases(const uint8_t *bases, size_t nbases, const uint8_t *scalars, size_t n, size_t off, size_t shift, int window_bits, uint8_t *out_xy, int *out_inf) {
    return guardk([&] {
        const char *who = "zkaes_msm_second_bases";
        need(out_xy && out_inf && (bases || !nbases) && (scalars || !n), who, "null argument");
        need(nbases <= MSM_FORM_MAX, who, "too many bases");
        if (window_bits) check_table_bits(window_bits, nbases, who);
        if (off > nbases || shift > nbases - off || n > nbases - off - shift) throw std::invalid_argument(window_bits ? "msm_table: range exceeds the table" : "zkaes_msm_second_bases: range exceeds the bases");
        run_msm_second_bases(bases, nbases, scalars, n, off, shift, window_bits, out_xy, out_inf);
    });
}
int zkaes_msm_sequence(const uint8_t *bases, size_t nbases, const uint8_t *scalars, size_t nscalars, const int8_t *class_vals, size_t nvals, const zkaes_msm_step *steps, size_t nsteps,
                       int poison, uint8_t *out_xy, int *out_inf, int *out_accepted, int *out_status, char *out_errors) {
    return guardk([&] {
        const char *who = "zkaes_msm_sequence";
        need(bases && steps && out_xy && out_inf && out_accepted && out_status && out_errors && (scalars || !nscalars) && (class_vals || !nvals), who, "null argument");
        need(nbases >= 1 && nbases <= MSM_FORM_MAX, who, "nbases out of range");
        need(nscalars <= MSM_FORM_MAX && nvals <= MSM_FORM_MAX, who, "too many scalars or class values");
        need(nsteps >= 1 && nsteps <= ZKAES_MSM_SEQ_MAX_STEPS, who, "1..32 steps");
        SeqBases forms;
        check_msm_sequence(steps, nsteps, nbases, nscalars, nvals, forms);
        run_msm_sequence(bases, nbases, scalars, nscalars, class_vals, nvals, steps, nsteps, poison != 0, forms, out_xy, out_inf, out_accepted, out_status, out_errors);
    });
}
int zkaes_msm_sharded_plan(int curve_id, size_t n_total, int *window_bits, int *n_windows, size_t *bytes_per_rank) {
    return guardk([&] {
        int c = 0, w = 0;
        if (curve_id == 381) zk::gpu::msm_sharded_plan<zk::Bls381>(n_total, &c, &w); else if (curve_id == 377) zk::gpu::msm_sharded_plan<zk::Bls377>(n_total, &c, &w); else throw std::invalid_argument("curve_id must be 377 or 381");
        if (window_bits) *window_bits = c;
        if (n_windows) *n_windows = w;
        if (bytes_per_rank) *bytes_per_rank = (size_t)w * 192;
    });
}
int zkaes_msm_window_sums_dev(int curve_id, const uint8_t *bases, const uint8_t *scalars, size_t n_local, size_t n_total, void *dev_out, size_t dev_out_bytes) {
    return guardk([&] { if (curve_id == 381) run_msm_window_sums_dev<zk::Bls381>(bases, scalars, n_local, n_total, dev_out, dev_out_bytes); else if (curve_id == 377) run_msm_window_sums_dev<zk::Bls377>(bases, scalars, n_local, n_total, dev_out, dev_out_bytes); else throw std::invalid_argument("curve_id must be 377 or 381"); });
}
int zkaes_msm_fold_window_sums_dev(int curve_id, const void *dev_in, int world, size_t n_total, uint8_t *out_xy, int *out_inf) {
    return guardk([&] { if (curve_id == 381) run_msm_fold_dev<zk::Bls381>(dev_in, world, n_total, out_xy, out_inf); else if (curve_id == 377) run_msm_fold_dev<zk::Bls377>(dev_in, world, n_total, out_xy, out_inf); else throw std::invalid_argument("curve_id must be 377 or 381"); });
}
int zkaes_g1_sum(int curve_id, const uint8_t *points_xy, const int *inf, size_t n, uint8_t *out_xy, int *out_inf) {
    return guardk([&] { if (curve_id == 381) run_g1_sum<zk::Bls381>(points_xy, inf, n, out_xy, out_inf); else if (curve_id == 377) run_g1_sum<zk::Bls377>(points_xy, inf, n, out_xy, out_inf); else throw std::invalid_argument("curve_id must be 377 or 381"); });
}
int zkaes_msm_fold_partials_dev(int curve_id, const void *dev_in, int world, uint8_t *out_xy, int *out_inf) {
    return guardk([&] {
        if (!dev_in || world < 1 || world > MAX_FOLD_WORLD) throw std::invalid_argument("zkaes_msm_fold_partials_dev: bad arguments (world must be 1..4096)");
        if (curve_id != 377 && curve_id != 381) throw std::invalid_argument("curve_id must be 377 or 381");
        zk::gpu::require_device();
        StreamGuard s;
        if (curve_id == 377) give_affine(zk::gpu::msm_fold_points_device<zk::Bls377>((const zk::XYZZ<zk::Fq377> *)dev_in, world, s).to_affine(), out_xy, out_inf);
        else give_affine(zk::gpu::msm_fold_points_device<zk::Bls381>((const zk::XYZZ<zk::Fq381> *)dev_in, world, s).to_affine(), out_xy, out_inf);
    });
}
int zkaes_msm_table(int curve_id, const uint8_t *bases, const uint8_t *scalars, size_t n, int window_bits, uint8_t *out_xy, int *out_inf) {
    return guardk([&] { if (curve_id == 381) run_msm_table<zk::Bls381, false>(bases, scalars, n, window_bits, out_xy, out_inf); else if (curve_id == 377) run_msm_table<zk::Bls377, false>(bases, scalars, n, window_bits, out_xy, out_inf); else throw std::invalid_argument("curve_id must be 377 or 381"); });
}
int zkaes_msm_table_srs(const uint8_t *bases, const uint8_t *scalars, size_t n, int window_bits, uint8_t *out_xy, int *out_inf) {
    return guardk([&] { run_msm_table<zk::Bls377, true>(bases, scalars, n, window_bits, out_xy, out_inf); });
}
int zkaes_set_device(int ordinal) { return guardk([&] { HIP_CHECK(hipSetDevice(ordinal)); }); }
int zkaes_ntt(int field_id, uint8_t *data, size_t n, int inverse) {
    return guardk([&] { if (field_id == 381) run_ntt<zk::Fr381>(data, n, inverse, 0, 0); else if (field_id == 377) run_ntt<zk::Fr377>(data, n, inverse, 0, 0); else throw std::invalid_argument("field_id must be 377 or 381"); });
}
int zkaes_ntt_coset(int field_id, uint8_t *data, size_t n, int inverse, int coset_c, int lg_big) {
    return guardk([&] {
        if (coset_c <= 0) throw std::invalid_argument("zkaes_ntt_coset: coset index must be positive");
        if (field_id == 381) run_ntt<zk::Fr381>(data, n, inverse, coset_c, lg_big); else if (field_id == 377) run_ntt<zk::Fr377>(data, n, inverse, coset_c, lg_big); else throw std::invalid_argument("field_id must be 377 or 381");
    });
}
int zkaes_ntt_batch(int field_id, uint8_t *data, size_t n, int count, int inverse, const int *coset_c, int lg_big) {
    return guardk([&] {
        if (field_id == 381) run_ntt_batch<zk::Fr381>(data, n, count, inverse, coset_c, lg_big); else if (field_id == 377) run_ntt_batch<zk::Fr377>(data, n, count, inverse, coset_c, lg_big);
        else throw std::invalid_argument("field_id must be 377 or 381");
    });
}
// ---- kernel-level entry points for tests (include/zkaes.h): BLS12-377 Fr unless a field_id says otherwise
int zkaes_poly_divide_by_vanishing(const uint8_t *p, size_t len, size_t m, int with_scratch, uint8_t *q, uint8_t *rem_or_null) {
    return guardk([&] {
        const char *who = "zkaes_poly_divide_by_vanishing";
        if (m == 0 || len <= m) throw std::invalid_argument("divide_by_vanishing: dividend shorter than divisor");
        need(p && q, who, "null argument"); need(len <= POLY_MAX, who, "polynomial too long");
        zk::gpu::require_device();
        StreamGuard s;
        DevPtr<PF> dp = upload(p, len, s), dq(len - m), drem(m), scratch;
        size_t scratch_len = 0;
        if (with_scratch) { scratch_len = zk::gpu::divide_by_vanishing_scratch(len, m); scratch.alloc(scratch_len ? scratch_len : 1); }
        zk::gpu::divide_by_vanishing(dq, rem_or_null ? drem.get() : nullptr, dp, len, m, s, with_scratch ? scratch.get() : nullptr, scratch_len);
        zk::gpu::d2h(q, dq, (len - m) * sizeof(PF), s);
        if (rem_or_null) zk::gpu::d2h(rem_or_null, drem, m * sizeof(PF), s);
    });
}
int zkaes_poly_divide_by_linear(const uint8_t *p, size_t len, const uint8_t z[32], uint8_t *q) {
    return guardk([&] {
        const char *who = "zkaes_poly_divide_by_linear";
        const PF zf = load_f(z, who);
        need(len <= POLY_MAX, who, "polynomial too long"); need(len < 2 || (p && q), who, "null argument");
        if (len < 2) return;                                   // a constant has the empty quotient
        zk::gpu::require_device();
        StreamGuard s;
        const size_t scratch_len = zk::gpu::divide_by_linear_scratch(len);
        DevPtr<PF> dp = upload(p, len, s), dq(len - 1), scratch(scratch_len);
        zk::gpu::divide_by_linear(dq, dp, len, zf, scratch, scratch_len, s);
        zk::gpu::d2h(q, dq, (len - 1) * sizeof(PF), s);
    });
}
int zkaes_poly_eval_multi(const uint8_t *const *polys, const size_t *lens, const uint8_t *x, int count, uint8_t *out) {
    return guardk([&] {
        const char *who = "zkaes_poly_eval_multi";
        need(count >= 1 && count <= 8, who, "1..8 polynomials"); need(polys && lens && x && out, who, "null argument");
        size_t scratch_len = 8;
        for (int i = 0; i < count; i++) { need(lens[i] <= POLY_MAX, who, "polynomial too long"); need(!lens[i] || polys[i], who, "null polynomial"); scratch_len += zk::gpu::poly_eval_scratch(lens[i]); }
        zk::gpu::require_device();
        StreamGuard s;
        DevPtr<PF> dp[8];
        const PF *ptr[8];
        PF xs[8], res[8];
        for (int i = 0; i < count; i++) { dp[i] = upload(polys[i], lens[i], s); ptr[i] = dp[i]; xs[i] = load_f(x + 32 * i, who); }
        DevPtr<PF> scratch(scratch_len);
        zk::gpu::poly_eval_multi(ptr, lens, xs, count, res, scratch, scratch_len, s);
        memcpy(out, res, (size_t)count * sizeof(PF));
    });
}
int zkaes_batch_inverse(uint8_t *v, size_t n, const uint8_t *post_or_null, int throughput_variant) {
    return guardk([&] {
        const char *who = "zkaes_batch_inverse";
        need(v || !n, who, "null argument"); need(n <= POLY_MAX, who, "vector too long");
        PF post; if (post_or_null) post = load_f(post_or_null, who);
        if (!n) return;
        zk::gpu::require_device();
        StreamGuard s;
        DevPtr<PF> dv = upload(v, n, s);
        {
            zk::gpu::ThroughputWaits as_between_overlapping_proofs(throughput_variant != 0);    // batch_inverse's own dispatch rule then takes the 16-element Fermat variant
            zk::gpu::batch_inverse(dv, n, post_or_null ? &post : nullptr, s);
            zk::gpu::sync(s);
        }
        zk::gpu::d2h(v, dv, n * sizeof(PF), s);
    });
}
int zkaes_poly_lincomb(const uint8_t *const *polys, const size_t *lens, const uint8_t *scalars, int count, size_t n, uint8_t *out) {
    return guardk([&] {
        const char *who = "zkaes_poly_lincomb";
        need(count >= 1 && count <= 8, who, "1..8 terms"); need(polys && lens && scalars && (out || !n), who, "null argument"); need(n <= POLY_MAX, who, "polynomial too long");
        for (int i = 0; i < count; i++) { need(lens[i] <= n, who, "a term longer than the result"); need(!lens[i] || polys[i], who, "null polynomial"); }
        if (!n) return;
        zk::gpu::require_device();
        StreamGuard s;
        DevPtr<PF> dp[8], dout(n);
        const PF *ptr[8];
        PF sc[8];
        for (int i = 0; i < count; i++) { dp[i] = upload(polys[i], lens[i], s); ptr[i] = dp[i]; sc[i] = load_f(scalars + 32 * i, who); }
        zk::gpu::poly_lincomb_n(dout, n, ptr, lens, sc, count, s);
        zk::gpu::d2h(out, dout, n * sizeof(PF), s);
    });
}
int zkaes_vanishing_quotient_evals(int lg_n, const uint8_t *g, int ncosets, const uint8_t a[32], const uint32_t *idx_or_null, size_t nidx, uint8_t *out) {
    return guardk([&] {
        const char *who = "zkaes_vanishing_quotient_evals";
        need(lg_n >= 0 && lg_n <= 24, who, "lg_n must be in [0, 24]"); need(ncosets >= 1 && ncosets <= 3, who, "1..3 cosets"); need(g && out, who, "null argument");
        const size_t n = (size_t)1 << lg_n;
        for (size_t i = 0; idx_or_null && i < nidx; i++) need(idx_or_null[i] < n, who, "index out of range");
        const PF af = load_f(a, who);
        PF gs[3];
        for (int c = 0; c < ncosets; c++) gs[c] = load_f(g + 32 * c, who);
        zk::gpu::require_device();
        StreamGuard s;
        const PF *elems = zk::gpu::domain_elements<zk::Fr377>(lg_n);
        const size_t scratch_len = zk::gpu::vanishing_quotient_scratch(lg_n, ncosets);
        DevPtr<PF> tabs[3], scratch(scratch_len);
        PF *outs[3] = {nullptr, nullptr, nullptr};
        for (int c = 0; c < ncosets; c++) { tabs[c].alloc(n); outs[c] = tabs[c]; }
        zk::gpu::vanishing_quotient_evals(outs, gs, ncosets, af, elems, (uint32_t)n, lg_n, scratch, scratch_len, s);
        if (!idx_or_null) { for (int c = 0; c < ncosets; c++) zk::gpu::d2h(out + (size_t)c * n * sizeof(PF), tabs[c], n * sizeof(PF), s); return; }
        std::vector<PF> host(n);
        for (int c = 0; c < ncosets; c++) {
            zk::gpu::d2h(host.data(), tabs[c], n * sizeof(PF), s);
            for (size_t i = 0; i < nidx; i++) memcpy(out + ((size_t)c * nidx + i) * sizeof(PF), &host[idx_or_null[i]], sizeof(PF));
        }
    });
}
int zkaes_q1_coset_pointwise(const uint8_t *r, const uint8_t *za, const uint8_t *zb, const uint8_t *t, const uint8_t *z, const uint8_t consts[192], size_t n, uint8_t *out) {
    return guardk([&] {
        const char *who = "zkaes_q1_coset_pointwise";
        need(r && za && zb && t && z && consts && out, who, "null argument"); need(n >= 1 && n <= POLY_MAX, who, "n out of range");
        PF c[6];
        for (int i = 0; i < 6; i++) c[i] = load_f(consts + 32 * i, who);
        zk::gpu::require_device();
        StreamGuard s;
        DevPtr<PF> dr = upload(r, n, s), dza = upload(za, n, s), dzb = upload(zb, n, s), dt = upload(t, n, s), dz = upload(z, n, s), dout(n);
        zk::gpu::q1_coset_pointwise(dout, dr, dza, dzb, dt, dz, c[0], c[1], c[2], c[3], c[4], c[5], n, s);
        zk::gpu::d2h(out, dout, n * sizeof(PF), s);
    });
}
int zkaes_h2_coset(const uint8_t *const arrays[7], const uint8_t consts[224], size_t k, uint8_t *out) {
    return guardk([&] {
        const char *who = "zkaes_h2_coset";
        need(arrays && consts && out, who, "null argument"); need(k >= 1 && k <= POLY_MAX, who, "k out of range");
        for (int i = 0; i < 7; i++) need(arrays[i], who, "null array");
        PF c[7];
        for (int i = 0; i < 7; i++) c[i] = load_f(consts + 32 * i, who);
        zk::gpu::require_device();
        StreamGuard s;
        DevPtr<PF> d[7], dout(k);
        for (int i = 0; i < 7; i++) d[i] = upload(arrays[i], k, s);
        zk::gpu::h2_coset(dout, d[0], d[1], d[2], d[3], d[4], d[5], d[6], c[0], c[1], c[2], c[3], c[4], c[5], c[6], k, s);
        zk::gpu::d2h(out, dout, k * sizeof(PF), s);
    });
}
int zkaes_q1_combine(const uint8_t *q0, const uint8_t *q1, const uint8_t *q3, const uint8_t *mask, const uint8_t inv2[32], const uint8_t inv2zeta[32], size_t n, uint8_t *h1, uint8_t *g1) {
    return guardk([&] {
        const char *who = "zkaes_q1_combine";
        need(q0 && q1 && q3 && mask && h1 && (g1 || n < 2), who, "null argument"); need(n >= 1 && n <= POLY_MAX / 4, who, "n out of range");
        const PF i2 = load_f(inv2, who), i2z = load_f(inv2zeta, who);
        zk::gpu::require_device();
        StreamGuard s;
        DevPtr<PF> d0 = upload(q0, n, s), d1 = upload(q1, n, s), d3 = upload(q3, n, s), dm = upload(mask, 3 * n, s), dh(2 * n), dg(n);
        zk::gpu::q1_combine(dh, dg, d0, d1, d3, dm, i2, i2z, n, s);
        zk::gpu::d2h(h1, dh, 2 * n * sizeof(PF), s);
        zk::gpu::d2h(g1, dg, (n - 1) * sizeof(PF), s);
    });
}
int zkaes_coset_scale(const uint8_t *in, size_t in_len, const uint8_t g[32], size_t n, uint8_t *out) {
    return guardk([&] {
        const char *who = "zkaes_coset_scale";
        need((in || !in_len) && (out || !n), who, "null argument"); need(n <= POLY_MAX && in_len <= POLY_MAX, who, "polynomial too long");
        const PF gf = load_f(g, who);
        if (!n) return;
        zk::gpu::require_device();
        StreamGuard s;
        DevPtr<PF> din = upload(in, in_len, s), dout(n);
        zk::gpu::coset_scale(dout, din, gf, in_len, n, s);
        zk::gpu::d2h(out, dout, n * sizeof(PF), s);
    });
}
int zkaes_z_poly_from_w(const uint8_t *w, size_t wlen, const uint8_t *x_poly, uint32_t m, size_t n, uint8_t *zp) {
    return guardk([&] {
        const char *who = "zkaes_z_poly_from_w";
        need((w || !wlen) && (x_poly || !m) && zp, who, "null argument"); need(n < POLY_MAX && wlen <= POLY_MAX, who, "polynomial too long");
        zk::gpu::require_device();
        StreamGuard s;
        DevPtr<PF> dw = upload(w, wlen, s), dx = upload(x_poly, m, s), dz(n + 1);
        zk::gpu::z_poly_from_w(dz, dw, wlen, dx, m, n, s);
        zk::gpu::d2h(zp, dz, (n + 1) * sizeof(PF), s);
    });
}
// ---- kernel-level entry points of the prover's R1CS and randomness kernels (include/zkaes.h): every argument is checked before anything is allocated or launched
int zkaes_spmv_bits(const uint32_t *rowptr, const uint32_t *col, const int64_t *coeff, size_t rows, size_t rows_out, const uint8_t *z, size_t ncols, uint8_t *out_field, int8_t *out_small_or_null) {
    return guardk([&] {
        const char *who = "zkaes_spmv_bits";
        need(rows_out >= 1 && rows_out <= R1CS_MAX, who, "rows_out out of range");
        need(rows <= rows_out, who, "rows must not exceed rows_out");
        need(ncols <= R1CS_MAX, who, "too many columns");
        need(out_field && (z || !ncols), who, "null argument");
        const size_t nnz = check_csr(rowptr, col, coeff, rows, ncols, who);
        zk::gpu::require_device();
        StreamGuard s;
        DevPtr<uint32_t> drp = upload_as(rowptr, rows + 1, s), dcol = upload_as(col, nnz, s);
        DevPtr<int64_t> dco = upload_as(coeff, nnz, s);
        DevPtr<uint8_t> dz = upload_as(z, ncols, s);
        DevPtr<PF> dout = poisoned<PF>(rows_out, s);
        DevPtr<int8_t> dsmall = poisoned<int8_t>(rows_out, s);
        zk::gpu::spmv_bits(dout, out_small_or_null ? dsmall.get() : nullptr, rows_out, drp, dcol, dco, rows, dz, s);
        zk::gpu::d2h(out_field, dout, rows_out * sizeof(PF), s);
        if (out_small_or_null) zk::gpu::d2h(out_small_or_null, dsmall, rows_out, s);
    });
}
int zkaes_w_maps(const uint8_t *z, size_t n, size_t m, size_t num_witness, const uint8_t *x_evals, int8_t *out_classes, uint8_t *out_w_evals, uint8_t *out_z_evals_h, uint8_t *out_x_field) {
    return guardk([&] {
        const char *who = "zkaes_w_maps";
        need(is_pow2(n) && is_pow2(m), who, "n and m must be powers of two");
        need(n <= R1CS_MAX, who, "n out of range");
        need(m < n, who, "m must be below n");
        need(num_witness <= n - m, who, "num_witness must not exceed n - m");
        need(z && x_evals && out_classes && out_w_evals && out_z_evals_h && out_x_field, who, "null argument");
        zk::gpu::require_device();
        StreamGuard s;
        DevPtr<uint8_t> dz = upload_as(z, m + num_witness, s);
        DevPtr<PF> dx = upload(x_evals, n, s), dw = poisoned<PF>(n, s), dzh = poisoned<PF>(n, s), dxf = poisoned<PF>(m, s);
        DevPtr<int8_t> dcl = poisoned<int8_t>(n, s);
        zk::gpu::w_classes(dcl, dz, (uint32_t)n, (uint32_t)m, (uint32_t)num_witness, s);
        zk::gpu::w_evals(dw, dz, dx, (uint32_t)n, (uint32_t)m, (uint32_t)num_witness, s);
        zk::gpu::z_evals_h(dzh, dz, (uint32_t)n, (uint32_t)m, (uint32_t)num_witness, s);
        zk::gpu::bits_to_field(dxf, dz, m, s);
        zk::gpu::d2h(out_classes, dcl, n, s);
        zk::gpu::d2h(out_w_evals, dw, n * sizeof(PF), s);
        zk::gpu::d2h(out_z_evals_h, dzh, n * sizeof(PF), s);
        zk::gpu::d2h(out_x_field, dxf, m * sizeof(PF), s);
    });
}
int zkaes_t_evals(size_t n, size_t m, size_t rows, const uint32_t *const rowptr[3], const uint32_t *const col[3], const int64_t *const coeff[3], const uint8_t *r_alpha,
                  const uint8_t etas[96], uint8_t *out, uint64_t stats[3]) {
    return guardk([&] {
        const char *who = "zkaes_t_evals";
        need(is_pow2(n) && is_pow2(m), who, "n and m must be powers of two");
        need(n <= R1CS_MAX, who, "n out of range");
        need(m < n, who, "m must be below n");
        need(rows <= n, who, "rows must not exceed n");
        need(rowptr && col && coeff && r_alpha && etas && out && stats, who, "null argument");
        zk::CsrMatrix M[3];
        size_t total = 0;
        for (int q = 0; q < 3; q++) {
            const size_t nnz = check_csr(rowptr[q], col[q], coeff[q], rows, n, who);
            total += nnz;
            M[q].rowptr.assign(rowptr[q], rowptr[q] + rows + 1);
            if (nnz) { M[q].col.assign(col[q], col[q] + nnz); M[q].coeff.assign(coeff[q], coeff[q] + nnz); }
        }
        need(total <= R1CS_MAX, who, "too many entries");
        PF eta[3];
        for (int q = 0; q < 3; q++) eta[q] = load_f(etas + 32 * q, who);
        const zk::hostx::TTables T = zk::hostx::build_t_tables(n, m, rows, M[0], M[1], M[2], zk::gpu::T_SEG, zk::gpu::T_HEAVY_SEGMENTS);       // the tables the prover's key holds
        uint32_t widest = 0;
        for (size_t h = 0; h < n; h++) widest = std::max(widest, T.col_seg_ptr[h + 1] - T.col_seg_ptr[h]);
        stats[0] = T.nseg; stats[1] = T.n_heavy; stats[2] = widest;
        zk::gpu::require_device();
        StreamGuard s;
        DevPtr<uint32_t> dcsp = upload_as(T.col_seg_ptr.data(), T.col_seg_ptr.size(), s), dss = upload_as(T.seg_start.data(), T.seg_start.size(), s),
                         dse = upload_as(T.seg_end.data(), T.seg_end.size(), s), dheavy = upload_as(T.heavy.data(), T.heavy.size(), s), drow = upload_as(T.trow.data(), T.trow.size(), s);
        DevPtr<uint8_t> dmat = upload_as(T.tmat.data(), T.tmat.size(), s);
        DevPtr<int64_t> dco = upload_as(T.tcoef.data(), T.tcoef.size(), s);
        DevPtr<PF> dra = upload(r_alpha, n, s), dout = poisoned<PF>(n, s), dpartial = poisoned<PF>(T.nseg, s);
        zk::gpu::t_evals(dout, (uint32_t)n, dpartial, T.nseg, dcsp, dss, dse, dheavy, T.n_heavy, drow, dmat, dco, dra, eta[0], eta[1], eta[2], s);
        zk::gpu::d2h(out, dout, n * sizeof(PF), s);
    });
}
int zkaes_lagrange_scalars(int lg_n, int lg_m, const uint8_t beta[32], uint8_t *out_lag, uint8_t *out_lag_w) {
    return guardk([&] {
        const char *who = "zkaes_lagrange_scalars";
        need(lg_n >= 1 && lg_n <= FR377_TWO_ADICITY, who, "lg_n must be in [1, the field's 2-adicity]");
        need(lg_m >= 0 && lg_m < lg_n, who, "lg_m must be in [0, lg_n)");
        need(lg_n <= 24, who, "lg_n must not exceed 24");
        need(out_lag && out_lag_w, who, "null argument");
        const PF b = load_f(beta, who);
        const size_t n = (size_t)1 << lg_n;
        zk::gpu::require_device();
        StreamGuard s;
        DevPtr<PF> dlag = poisoned<PF>(n, s), dlagw = poisoned<PF>(n, s);
        zk::gpu::lagrange_scalars(dlag, dlagw, zk::gpu::domain_elements<zk::Fr377>(lg_n), b, (uint32_t)n, 1u << lg_m, s);
        zk::gpu::d2h(out_lag, dlag, n * sizeof(PF), s);
        zk::gpu::d2h(out_lag_w, dlagw, n * sizeof(PF), s);
    });
}
int zkaes_f_evals_from_tables(const uint8_t *va, const uint8_t *vb, const uint8_t *vc, const uint8_t ea[32], const uint8_t eb[32], const uint8_t ec[32], const uint8_t *ra, const uint8_t *rb,
                              const uint32_t *ri, const uint32_t *ci, size_t k, size_t n, uint8_t *out) {
    return guardk([&] {
        const char *who = "zkaes_f_evals_from_tables";
        need(k >= 1 && k <= R1CS_MAX && n >= 1 && n <= R1CS_MAX, who, "k or n out of range");
        need(va && vb && vc && ra && rb && ri && ci && out, who, "null argument");
        const PF fa = load_f(ea, who), fb = load_f(eb, who), fc = load_f(ec, who);
        for (size_t i = 0; i < k; i++) need(ri[i] < n && ci[i] < n, who, "index out of range");
        zk::gpu::require_device();
        StreamGuard s;
        DevPtr<PF> dva = upload(va, k, s), dvb = upload(vb, k, s), dvc = upload(vc, k, s), dra = upload(ra, n, s), drb = upload(rb, n, s), dout = poisoned<PF>(k, s);
        DevPtr<uint32_t> dri = upload_as(ri, k, s), dci = upload_as(ci, k, s);
        zk::gpu::f_evals_from_tables(dout, dva, dvb, dvc, fa, fb, fc, dra, drb, dri, dci, k, s);
        zk::gpu::d2h(out, dout, k * sizeof(PF), s);
    });
}
int zkaes_chacha_field_stream(const uint32_t key_words[8], int rounds, uint64_t word_pos, size_t count, uint32_t max_cand, uint8_t *out, uint64_t *next_word_pos) {
    return guardk([&] {
        const char *who = "zkaes_chacha_field_stream";
        need(key_words && next_word_pos && (out || !count), who, "null argument");
        need(rounds == 8 || rounds == 12 || rounds == 20, who, "rounds must be 8, 12 or 20");
        need(count <= R1CS_MAX, who, "count out of range");
        need(word_pos <= ~(uint64_t)0 - 64 * (uint64_t)R1CS_MAX, who, "word_pos too close to the end of the stream");
        zk::gpu::require_device();
        StreamGuard s;
        // chacha_field_stream: a batch has at most count / 0.58 * 1.02 + 4096 candidates of 8 words, its blocks, a flag and a position per candidate and 1 MB for the scan
        const size_t ncand = 2 * count + 8192, scratch_bytes = (ncand * 8 / 16 + 4) * 64 + ncand * 8 + ((size_t)4 << 20);
        DevPtr<void> scratch = poisoned<void>(scratch_bytes, s);
        DevPtr<PF> dout = poisoned<PF>(count, s);
        *next_word_pos = zk::gpu::chacha_field_stream(dout, count, key_words, rounds, word_pos, scratch, scratch_bytes, s, max_cand);
        zk::gpu::d2h(out, dout, count * sizeof(PF), s);
    });
}
int zkaes_mask_fixup(uint8_t *p, size_t n) {
    return guardk([&] {
        const char *who = "zkaes_mask_fixup";
        need(n >= 1 && n <= R1CS_MAX, who, "n out of range");
        need(p != nullptr, who, "null argument");
        zk::gpu::require_device();
        StreamGuard s;
        DevPtr<PF> dp = upload(p, 3 * n, s);
        zk::gpu::mask_fixup(dp, n, s);
        zk::gpu::d2h(p, dp, 3 * n * sizeof(PF), s);
    });
}
// ---- kernel-level entry points of the kernels that build a key (include/zkaes.h): every argument is checked before anything is allocated or launched
int zkaes_fixed_base_powers(int curve_id, const uint8_t base_xy[96], const uint8_t beta[32], uint64_t from, size_t count, size_t chunk, uint8_t *out) {
    return guardk([&] {
        const char *who = "zkaes_fixed_base_powers";
        need(curve_id == 377 || curve_id == 381, who, "curve_id must be 377 or 381");
        need(base_xy && beta && (out || !count), who, "null argument");
        need(count <= KEYSYNTH_MAX && chunk <= KEYSYNTH_MAX, who, "count or chunk out of range");
        need(from <= ~(uint64_t)0 - KEYSYNTH_MAX, who, "from too close to 2^64");
        if (!count) return;
        if (curve_id == 377) run_fixed_base_powers<zk::Bls377>(base_xy, beta, from, count, chunk, out); else run_fixed_base_powers<zk::Bls381>(base_xy, beta, from, count, chunk, out);
    });
}
int zkaes_fixed_base_scalars(const uint8_t base_xy[96], const uint8_t *scalars, size_t count, size_t chunk, uint8_t *out) {
    return guardk([&] {
        const char *who = "zkaes_fixed_base_scalars";
        need(base_xy && (scalars || !count) && (out || !count), who, "null argument");
        need(count <= KEYSYNTH_MAX && chunk <= KEYSYNTH_MAX, who, "count or chunk out of range");
        if (!count) return;
        zk::gpu::require_device();
        StreamGuard s;
        DevPtr<MFr> ds = upload_scalars(scalars, count, s);
        DevPtr<zk::Affine<MFq>> d = poisoned<zk::Affine<MFq>>(count, s);
        zk::gpu::fixed_base_scalars<MC>(d, load_point<MFq>(base_xy), ds, count, s, chunk);
        zk::gpu::d2h(out, d, count * 96, s);
    });
}
int zkaes_table_next(int curve_id, const uint8_t *prev, size_t count, int window_bits, int j, uint8_t *out) {
    return guardk([&] {
        const char *who = "zkaes_table_next";
        check_curve_table_args(curve_id, window_bits, count, who);
        need(prev && out, who, "null argument");
        const int nt = curve_id == 377 ? zk::gpu::table_windows<zk::Bls377>(window_bits) : zk::gpu::table_windows<zk::Bls381>(window_bits);
        need(j >= 1 && j < nt, who, "j must be in [1, table copies)");
        if (curve_id == 377) run_table_next<zk::Bls377>(prev, count, window_bits, j, out); else run_table_next<zk::Bls381>(prev, count, window_bits, j, out);
    });
}
int zkaes_build_window_tables(int curve_id, const uint8_t *bases, size_t n, int window_bits, uint8_t *out) {
    return guardk([&] {
        const char *who = "zkaes_build_window_tables";
        check_curve_table_args(curve_id, window_bits, n, who);
        need(bases && out, who, "null argument");
        if (curve_id == 377) run_build_window_tables<zk::Bls377>(bases, n, window_bits, out); else run_build_window_tables<zk::Bls381>(bases, n, window_bits, out);
    });
}
int zkaes_convert_bases_te(const uint8_t *src, size_t n, uint8_t *out) {
    return guardk([&] {
        const char *who = "zkaes_convert_bases_te";
        static_assert(sizeof(zk::Niels28<MP>) == ZKAES_NIELS_RECORD_BYTES, "the record size the header states");
        need(n >= 1 && n <= KEYSYNTH_MAX, who, "n out of range");
        need(src && out, who, "null argument");
        zk::gpu::require_device();
        StreamGuard s;
        DevPtr<zk::Affine<MFq>> db = upload_points(src, n, n, s);
        DevPtr<zk::Niels28<MP>> dn = poisoned<zk::Niels28<MP>>(n, s);
        zk::gpu::convert_bases_te<MC>(dn, db, n, s);
        zk::gpu::d2h(out, dn, n * sizeof(zk::Niels28<MP>), s);
    });
}
int zkaes_index_evals(const uint32_t *ci, const uint32_t *ri, const int64_t *ca, const int64_t *cb, const int64_t *cc, size_t cnt, int lg_k, int lg_n, uint8_t *row, uint8_t *col, uint8_t *rowcol,
                      uint8_t *va, uint8_t *vb, uint8_t *vc, uint8_t *uinv_or_null) {
    return guardk([&] {
        const char *who = "zkaes_index_evals";
        need(lg_n >= 0 && lg_n <= 20 && lg_k >= 0 && lg_k <= 20, who, "lg_n and lg_k must be in [0, 20]");
        const size_t k = (size_t)1 << lg_k, n = (size_t)1 << lg_n, room = k + ZKAES_INDEX_EVALS_TAIL;
        need(cnt <= k, who, "cnt must not exceed k");
        need(row && col && rowcol && va && vb && vc && (!cnt || (ci && ri && ca && cb && cc)), who, "null argument");
        for (size_t i = 0; i < cnt; i++) need(ci[i] < n && ri[i] < n, who, "index out of range");
        zk::gpu::require_device();
        StreamGuard s;
        DevPtr<uint32_t> dci = upload_as(ci, cnt, s), dri = upload_as(ri, cnt, s);
        DevPtr<int64_t> dca = upload_as(ca, cnt, s), dcb = upload_as(cb, cnt, s), dcc = upload_as(cc, cnt, s);
        DevPtr<PF> d[7];
        for (int i = 0; i < 7; i++) d[i] = poisoned<PF>(room, s);
        zk::gpu::index_evals(d[0], d[1], d[2], d[3], d[4], d[5], d[6], dci, dri, dca, dcb, dcc, cnt, k, zk::gpu::domain_elements<zk::Fr377>(lg_n), (uint32_t)n, s);
        uint8_t *outs[7] = {row, col, rowcol, va, vb, vc, uinv_or_null};
        for (int i = 0; i < 7; i++) if (outs[i]) zk::gpu::d2h(outs[i], d[i], room * sizeof(PF), s);
    });
}
int zkaes_ntt_padded(int field_id, const uint8_t *in, size_t in_len, size_t n, int inverse, int coset_c, int lg_big, uint8_t *out) {
    return guardk([&] {
        if (field_id == 381) run_ntt_padded<zk::Fr381>(in, in_len, n, inverse, coset_c, lg_big, out); else if (field_id == 377) run_ntt_padded<zk::Fr377>(in, in_len, n, inverse, coset_c, lg_big, out);
        else throw std::invalid_argument("field_id must be 377 or 381");
    });
}
int zkaes_ntt_scaled(const uint8_t g[32], const uint8_t *in, size_t in_len, size_t n, int inverse, uint8_t *out) {
    return guardk([&] {
        const char *who = "zkaes_ntt_scaled";
        const int lg = exact_log2(n, who);
        need(lg >= 1 && lg <= 28, who, "n must be in [2, 2^28]"); need(in_len <= n, who, "in_len must not exceed n"); need(out && (in || !in_len), who, "null argument");
        const PF gf = load_f(g, who);
        need(!gf.is_zero(), who, "the coset generator must not be zero");
        zk::gpu::require_device();
        StreamGuard s;
        DevPtr<void> table = zk::gpu::coset_power_table<PF>(inverse ? gf.inverse() : gf, n, s);      // g^i evaluates on g D, g^-i interpolates from there
        DevPtr<PF> a = upload(in, in_len, s), b(n);
        zk::gpu::ntt_scaled<PF>(b, a, in_len, lg, inverse != 0, table, s);
        zk::gpu::d2h(out, b, n * sizeof(PF), s);
    });
}
int zkaes_msm(int curve_id, const uint8_t *bases, const uint8_t *scalars, size_t n, uint8_t *out_xy, int *out_inf) {
    return guardk([&] { if (curve_id == 381) run_msm<zk::Bls381>(bases, scalars, n, out_xy, out_inf, 0, nullptr, nullptr); else if (curve_id == 377) run_msm<zk::Bls377>(bases, scalars, n, out_xy, out_inf, 0, nullptr, nullptr); else throw std::invalid_argument("curve_id must be 377 or 381"); });
}
int zkaes_msm_bench(int curve_id, const uint8_t *bases, const uint8_t *scalars, size_t n, int reps, double *ms_total, double *ms_accumulate) {
    return guardk([&] { if (curve_id == 381) run_msm<zk::Bls381>(bases, scalars, n, nullptr, nullptr, reps, ms_total, ms_accumulate); else run_msm<zk::Bls377>(bases, scalars, n, nullptr, nullptr, reps, ms_total, ms_accumulate); });
}
// BLS12-377 only: n_points synthetic bases (powers of a fixed scalar times the generator, made on the device) and pseudo-random scalars;
// window_bits = 0 -> per-window buckets on the Weierstrass model (the generic path), < 0 -> per-window buckets on the twisted Edwards model (the prover's lone-call
// path), > 0 -> the precomputed-table path (Edwards).  Returns ms per MSM (whole pipeline / accumulate kernel).
int zkaes_msm_bench_synth(size_t n, int window_bits, int reps, double *ms_total, double *ms_accumulate, uint8_t *out_xy) {
    return guardk([&] {
        using Fq = zk::Fq377; using Fr = zk::Fr377;
        if (!ms_total || !ms_accumulate || reps < 1 || n == 0 || window_bits > 22) throw std::invalid_argument("zkaes_msm_bench_synth: bad arguments");
        zk::gpu::require_device();
        const size_t nt = window_bits > 0 ? (size_t)zk::gpu::table_windows<zk::Bls377>(window_bits) : 1;
        if ((uint64_t)nt * n >= (1ull << 30)) throw std::invalid_argument("zkaes_msm_bench_synth: n x table copies exceeds the 2^30 base indices of one MSM");
        StreamGuard s;
        DevPtr<zk::Affine<Fq>> tab(nt * n);
        zk::Affine<Fq> g; for (int i = 0; i < 12; i++) { g.x.l[i] = G1_377_X_MONT[i]; g.y.l[i] = G1_377_Y_MONT[i]; }
        Fr beta = Fr::from_u64(0x9e3779b97f4a7c15ull) * Fr::from_u64(0xc2b2ae3d27d4eb4full);
        zk::gpu::fixed_base_powers<zk::Bls377>(tab, g, beta, 1, n, s);
        if (window_bits > 0) zk::gpu::build_window_tables<zk::Bls377>(tab, n, window_bits, s);
        // window_bits == 0: the generic path (Weierstrass model, XYZZ buckets, 112-byte bases); < 0 or > 0: the prover's SRS path on the twisted Edwards model
        const bool edwards = window_bits != 0;
        DevPtr<zk::Affine28<zk::Fq377P>> tab28;
        DevPtr<zk::Niels28<zk::Fq377P>> tabte;
        if (edwards) { tabte.alloc(nt * n); zk::gpu::convert_bases_te<zk::Bls377>(tabte, tab, nt * n, s); }
        else { tab28.alloc(nt * n); zk::gpu::convert_bases<zk::Bls377>(tab28, tab, nt * n, s); }
        std::vector<Fr> sc(n);
        uint64_t x = 88172645463325252ull;
        for (size_t i = 0; i < n; i++) { for (int k = 0; k < 8; k += 2) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; sc[i].l[k] = (uint32_t)x; sc[i].l[k + 1] = (uint32_t)(x >> 32); } sc[i].l[7] &= 0x0fffffffu; }
        DevPtr<Fr> ds(n);
        zk::gpu::h2d(ds, sc.data(), n * 32, s);
        zk::gpu::sync(s);
        WorkspaceGuard ws;
        auto run = [&]() -> zk::XYZZ<Fq> {
            if (edwards) return window_bits > 0 ? zk::gpu::msm_table<zk::Bls377>(ws, tabte, n, 0, window_bits, ds, n, s) : zk::gpu::msm<zk::Bls377>(ws, tabte.get(), ds.get(), n, s);
            return window_bits > 0 ? zk::gpu::msm_table<zk::Bls377>(ws, tab28, n, 0, window_bits, ds, n, s) : zk::gpu::msm<zk::Bls377>(ws, tab28.get(), ds.get(), n, s);
        };
        give_affine(run().to_affine(), out_xy, nullptr);
        zk::gpu::MsmStats before = zk::gpu::msm_stats(false);
        EventGuard e0, e1;
        zk::gpu::event_record(e0, s);
        for (int i = 0; i < reps; i++) run();
        zk::gpu::event_record(e1, s);
        float ms = zk::gpu::event_elapsed_ms(e0, e1);
        zk::gpu::MsmStats after = zk::gpu::msm_stats(false);
        *ms_total = ms / reps; *ms_accumulate = (after.accumulate_ms - before.accumulate_ms) / reps;
    });
}

int zkaes_stream_copy_bench(size_t bytes, int reps, double *gb_per_s) {
    return guardk([&] {
        if (bytes < 4096 || reps < 1 || !gb_per_s) throw std::invalid_argument("zkaes_stream_copy_bench: bytes >= 4096, reps >= 1");
        zk::gpu::require_device();
        StreamGuard s;
        const size_t n16 = bytes / 16;
        DevPtr<uint4> a(n16), b(n16);
        zk::gpu::dzero(a, n16 * 16, s);
        hipStream_t hs = (hipStream_t)s.h;
        k_stream_copy<<<(unsigned)((n16 + 1023) / 1024), 256, 0, hs>>>(b, a, n16);
        EventGuard e0, e1;
        zk::gpu::event_record(e0, s);
        for (int i = 0; i < reps; i++) k_stream_copy<<<(unsigned)((n16 + 1023) / 1024), 256, 0, hs>>>(i & 1 ? a.get() : b.get(), i & 1 ? b.get() : a.get(), n16);
        zk::gpu::event_record(e1, s);
        float ms = zk::gpu::event_elapsed_ms(e0, e1);
        *gb_per_s = 2.0 * (double)(n16 * 16) * reps / 1e9 / (ms / 1e3);   // read + write
    });
}
int zkaes_int_rate_bench(double seconds, double out[8]) {
    return guardk([&] {
        if (!out || !(seconds > 0.0) || seconds > 30.0) throw std::invalid_argument("zkaes_int_rate_bench: 0 < seconds <= 30, out != NULL");
        zk::gpu::require_device();
        using P = zk::Fq377P; using G = zk::FpMsm<P>;
        StreamGuard s;
        hipStream_t hs = (hipStream_t)s.h;
        const int GRID_A = 4096, ITERS_A = 300, GRID_B = 8192, ITERS_B = 83;      // A: 4 waves per SIMD, 600 products per lane; B: k_accumulate's launch shape for 2^19 buckets of ~83 points
        const uint32_t NREC = 4096;                                                // 768 KB of records: L2-resident
        DevPtr<CalStamp> st(GRID_B);
        DevPtr<G> sink_a((size_t)GRID_A * 64);
        DevPtr<zk::AccTE<P>> sink_b((size_t)GRID_B * 64);
        DevPtr<zk::Niels28<P>> tab(NREC);
        k_cal_fill<<<NREC / 256, 256, 0, hs>>>(tab, NREC);
        G ga; for (int k = 0; k < 14; k++) ga.l[k] = 0x0123457u + 977u * k;
        std::vector<double> rate_a, mhz_a, rate_b, mhz_b, cyc_b;
        std::vector<CalStamp> h(GRID_B);
        auto median = [](std::vector<double> &v) { std::sort(v.begin(), v.end()); return v.empty() ? 0.0 : v[v.size() / 2]; };
        auto stamps = [&](int grid, double per_wave_units, double *mhz, double *cyc_per_unit) {
            zk::gpu::d2h(h.data(), st, (size_t)grid * sizeof(CalStamp), s);
            std::vector<double> m(grid), c(grid);
            for (int i = 0; i < grid; i++) { m[i] = (double)h[i].cyc / ((double)h[i].rt / 1e8) / 1e6; c[i] = (double)h[i].cyc / per_wave_units; }
            *mhz = median(m); *cyc_per_unit = median(c);
        };
        EventGuard e0, e1;
        const auto t_begin = std::chrono::steady_clock::now();
        int rounds = 0;
        // warm-up launches are part of the loop: the first rounds run while the clocks settle and the median discards them
        while (rounds < 3 || std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count() < seconds) {
            double mhz, cyc;
            zk::gpu::event_record(e0, s);
            k_cal_fqmul<<<GRID_A, 64, 0, hs>>>(st, sink_a, ga, ITERS_A);
            zk::gpu::event_record(e1, s);
            stamps(GRID_A, 2.0 * ITERS_A, &mhz, &cyc);
            rate_a.push_back(2.0 * ITERS_A * 64.0 * GRID_A / (zk::gpu::event_elapsed_ms(e0, e1) * 1e-3)); mhz_a.push_back(mhz);
            zk::gpu::event_record(e0, s);
            k_cal_hot_loop<<<GRID_B, 64, 0, hs>>>(st, sink_b, tab, NREC - 1, ITERS_B);
            zk::gpu::event_record(e1, s);
            stamps(GRID_B, (double)ITERS_B, &mhz, &cyc);
            rate_b.push_back((double)ITERS_B * 64.0 * GRID_B / (zk::gpu::event_elapsed_ms(e0, e1) * 1e-3)); mhz_b.push_back(mhz); cyc_b.push_back(cyc);
            rounds++;
        }
        out[0] = median(rate_a); out[1] = median(mhz_a); out[2] = median(rate_b); out[3] = median(mhz_b); out[4] = median(cyc_b); out[5] = (double)rounds; out[6] = 0; out[7] = 0;
    });
}
int zkaes_mem_info(uint64_t *free_bytes, uint64_t *total_bytes) {
    return guardk([&] {
        zk::gpu::require_device();
        size_t f = 0, t = 0;
        HIP_CHECK(hipMemGetInfo(&f, &t));
        if (free_bytes) *free_bytes = f;
        if (total_bytes) *total_bytes = t;
    });
}
}
