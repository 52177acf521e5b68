// csrc/arith_probe.cuh -- ONE operation of ff.cuh / ff28.cuh / ff29.cuh / ec28.cuh / te28.cuh per probe, raw limbs in and raw limbs out (TEST-ONLY).
//
// The field and curve headers take a different code path on the device than on the host (32-bit against 64-bit CIOS, v_sad_u32 against the plain expression, __umulhi
// against a 64-bit shift, an opaque SGPR bias, DPP quad moves), and the kernels reach those paths only through whole MSMs and NTTs.  A probe runs a single operation on
// operands given as uint32_t limb arrays EXACTLY as the operation sees them -- no conversion on the way in or out, so lazy limbs above 28 / 29 bits and non-canonical
// representatives can be passed -- and the same body is compiled for the device (capi_probe.hip: one kernel per operation) and for the host (tests/arith_probe_host.cpp).
// tests/arith_model.py holds the big-integer model both are compared with.
//
// An operation is a struct with NIN / NOUT (32-bit words per case) and run(in, out, bias); the four-lanes-per-point forms have QUAD = true and run_quad(in, out, q), device
// only.  ZK_PROBE_OPS lists (id, type): the ids are the `op` argument of zkaes_arith_probe, and api.py ARITH_OPS names them.
#pragma once
#include "ff29.cuh"
#include "te28.cuh"

namespace zk {
namespace probe {

template <class T> ZK_HD T ld(const uint32_t *in) { T r; for (int i = 0; i < T::N; i++) r.l[i] = in[i]; return r; }
template <class T> ZK_HD void st(uint32_t *out, const T &v) { for (int i = 0; i < T::N; i++) out[i] = v.l[i]; }
struct OpBase { static constexpr bool QUAD = false, SEEDED = false; };      // SEEDED: has run_seeded(in, out, seed) for the kernel that took hot_loop_seed() at its entry

// ---- unary / binary shapes shared by the three field classes: T -> T and T x T -> T
#define ZK_PROBE_UN(NAME, EXPR)                                                                                                                   \
    template <class T> struct NAME : OpBase { static constexpr int NIN = T::N, NOUT = T::N;                                                       \
        ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) { const T a = ld<T>(in); st<T>(out, EXPR); } };
#define ZK_PROBE_BIN(NAME, EXPR)                                                                                                                  \
    template <class T> struct NAME : OpBase { static constexpr int NIN = 2 * T::N, NOUT = T::N;                                                   \
        ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) { const T a = ld<T>(in), b = ld<T>(in + T::N); st<T>(out, EXPR); } };
#define ZK_PROBE_BIN_K(NAME, EXPR)                                                                                                                \
    template <class T, int K> struct NAME : OpBase { static constexpr int NIN = 2 * T::N, NOUT = T::N;                                            \
        ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) { const T a = ld<T>(in), b = ld<T>(in + T::N); st<T>(out, EXPR); } };
ZK_PROBE_BIN(Mul, a * b)
ZK_PROBE_BIN(Add, a + b)
ZK_PROBE_BIN(Sub, a - b)                               // Fp<P> only
ZK_PROBE_UN(Neg, a.neg())
ZK_PROBE_UN(Dbl, a.dbl())
ZK_PROBE_UN(Inverse, a.inverse())
ZK_PROBE_UN(FromRaw, T::from_raw(a.l))
ZK_PROBE_UN(Sqr, a.sqr())
ZK_PROBE_BIN(AddLazy, a.add_lazy(b))
ZK_PROBE_UN(DblLazy, a.dbl_lazy())
ZK_PROBE_BIN_K(SubK, a.template sub<K>(b))
ZK_PROBE_BIN_K(SubLazyK, a.template sub_lazy<K>(b))
ZK_PROBE_UN(Canonical, a.canonical())                  // Fp28
ZK_PROBE_UN(Normalized, a.normalized())                // Fp29 from here
ZK_PROBE_UN(Shl5, a.shl5())
ZK_PROBE_UN(ReduceTop, a.reduce_by_top_limb())
template <class T, int LOG> struct CanonicalLog : OpBase { static constexpr int NIN = T::N, NOUT = T::N;
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) { st<T>(out, ld<T>(in).template canonical<LOG>()); } };

// ---- Fp<P>: the rest
template <class F> struct ToRaw : OpBase { static constexpr int NIN = F::N, NOUT = F::N;
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) { ld<F>(in).to_raw(out); } };
template <class F> struct FromI64 : OpBase { static constexpr int NIN = 2, NOUT = F::N;       // the two's-complement value, low word first
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) { st<F>(out, F::from_i64((int64_t)((uint64_t)in[0] | (uint64_t)in[1] << 32))); } };
template <class F> struct PowU64 : OpBase { static constexpr int NIN = F::N + 2, NOUT = F::N;
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) { st<F>(out, ld<F>(in).pow_u64((uint64_t)in[F::N] | (uint64_t)in[F::N + 1] << 32)); } };

// ---- Fp28<P>: the rest
template <class G> struct Fma2 : OpBase { static constexpr int NIN = 4 * G::N, NOUT = G::N;
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) { st<G>(out, G::fma2(ld<G>(in), ld<G>(in + G::N), ld<G>(in + 2 * G::N), ld<G>(in + 3 * G::N))); } };
template <class G> struct ProductIsZero : OpBase { static constexpr int NIN = G::N, NOUT = 1;
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) { out[0] = G::product_is_zero(ld<G>(in)) ? 1u : 0u; } };
template <class G> struct IsZeroModP : OpBase { static constexpr int NIN = G::N, NOUT = 1;
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) { out[0] = ld<G>(in).is_zero_mod_p() ? 1u : 0u; } };
template <class P> struct FromStd28 : OpBase { static constexpr int NIN = P::N, NOUT = 14;
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) { st<Fp28<P>>(out, Fp28<P>::from_std(ld<Fp<P>>(in))); } };
template <class P> struct ToStd28 : OpBase { static constexpr int NIN = 14, NOUT = P::N;
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) { st<Fp<P>>(out, ld<Fp28<P>>(in).to_std()); } };
template <class G> struct MulBiased : OpBase { static constexpr int NIN = 2 * G::N, NOUT = G::N;
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t bias) { st<G>(out, G::mul_biased(ld<G>(in), ld<G>(in + G::N), bias)); } };

// ---- Fp29<P>: the rest
template <class S, int M> struct Dot : OpBase { static constexpr int NIN = 2 * M * S::N, NOUT = S::N;      // a[0..M), then b[0..M)
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) {
        S a[M], b[M];
        for (int i = 0; i < M; i++) { a[i] = ld<S>(in + i * S::N); b[i] = ld<S>(in + (M + i) * S::N); }
        st<S>(out, S::template dot<M>(a, b));
    } };
template <class P> struct TwiddleFromStd : OpBase { static constexpr int NIN = P::N, NOUT = 9;
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) { st<Fp29<P>>(out, Fp29<P>::twiddle_from_std(ld<Fp<P>>(in))); } };
template <class P> struct Split29 : OpBase { static constexpr int NIN = P::N, NOUT = 9;
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) { st<Fp29<P>>(out, Fp29<P>::split(in)); } };
template <class P> struct Pack29 : OpBase { static constexpr int NIN = 9, NOUT = P::N;
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) { ld<Fp29<P>>(in).pack(out); } };

// ---- points: coordinates in the struct's order, 14 limbs each (x y z t / x y zz zzz / ymx ypx td), XYZZ<Fp> and Affine<Fp> 12 words each
constexpr int GW = 14, PTW = 4 * GW, NIW = 3 * GW;
template <class P> ZK_HD AccTE<P> ld_te(const uint32_t *in) { AccTE<P> a; a.x = ld<FpMsm<P>>(in); a.y = ld<FpMsm<P>>(in + GW); a.z = ld<FpMsm<P>>(in + 2 * GW); a.t = ld<FpMsm<P>>(in + 3 * GW); return a; }
template <class P> ZK_HD void st_te(uint32_t *out, const AccTE<P> &a) { st(out, a.x); st(out + GW, a.y); st(out + 2 * GW, a.z); st(out + 3 * GW, a.t); }
template <class P> ZK_HD Acc28<P> ld_acc(const uint32_t *in) { Acc28<P> a; a.x = ld<FpMsm<P>>(in); a.y = ld<FpMsm<P>>(in + GW); a.zz = ld<FpMsm<P>>(in + 2 * GW); a.zzz = ld<FpMsm<P>>(in + 3 * GW); return a; }
template <class P> ZK_HD void st_acc(uint32_t *out, const Acc28<P> &a) { st(out, a.x); st(out + GW, a.y); st(out + 2 * GW, a.zz); st(out + 3 * GW, a.zzz); }
template <class P> ZK_HD Niels28<P> ld_niels(const uint32_t *in) {
    Niels28<P> n; n.ymx = ld<FpMsm<P>>(in); n.ypx = ld<FpMsm<P>>(in + GW); n.td = ld<FpMsm<P>>(in + 2 * GW);
    for (int i = 0; i < 6; i++) n.pad[i] = 0;
    return n;
}
template <class P> ZK_HD void st_niels(uint32_t *out, const Niels28<P> &n) { st(out, n.ymx); st(out + GW, n.ypx); st(out + 2 * GW, n.td); }
template <class P> ZK_HD void st_xyzz(uint32_t *out, const XYZZ<Fp<P>> &o) { st(out, o.x); st(out + P::N, o.y); st(out + 2 * P::N, o.zz); st(out + 3 * P::N, o.zzz); }

struct TeMadd : OpBase { using P = Fq377P; static constexpr int NIN = PTW + NIW, NOUT = PTW;
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) { AccTE<P> a = ld_te<P>(in); te_madd<P>(a, ld_niels<P>(in + PTW)); st_te<P>(out, a); } };
struct TeAdd : OpBase { using P = Fq377P; static constexpr int NIN = 2 * PTW, NOUT = PTW;
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) { AccTE<P> a = ld_te<P>(in); te_add<P>(a, ld_te<P>(in + PTW)); st_te<P>(out, a); } };
struct TeDbl : OpBase { using P = Fq377P; static constexpr int NIN = PTW, NOUT = PTW;
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) { AccTE<P> a = ld_te<P>(in); te_dbl<P>(a); st_te<P>(out, a); } };
struct TeNeg : OpBase { using P = Fq377P; static constexpr int NIN = PTW, NOUT = PTW;
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) { st_te<P>(out, te_neg<P>(ld_te<P>(in))); } };
struct TeToStd : OpBase { using P = Fq377P; static constexpr int NIN = PTW, NOUT = 4 * P::N;
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) { st_xyzz<P>(out, te_to_std_point<P>(ld_te<P>(in))); } };
// Weierstrass affine (x, y: 12 words each) -> the table record, then the `bad` flag
struct NielsFromW : OpBase { using P = Fq377P; static constexpr int NIN = 2 * P::N, NOUT = NIW + 1;
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) {
        Affine<Fp<P>> p; p.x = ld<Fp<P>>(in); p.y = ld<Fp<P>>(in + P::N);
        bool bad = false;
        st_niels<P>(out, niels_from_weierstrass(p, &bad));
        out[NIW] = bad ? 1u : 0u;
    } };
// in: accumulator, the current record AS LOADED (niels_load_signed with the current sign), the next record as it lies in the table, neg, next_neg;
// out: accumulator, then the record left in n (the next one, loaded with ITS sign)
struct TeMaddHot : OpBase { using P = Fq377P; static constexpr bool SEEDED = true; static constexpr int NIN = PTW + 2 * NIW + 2, NOUT = PTW + NIW;
    ZK_HD static void run_seeded(const uint32_t *in, uint32_t *out, FpMsm<P>::Seed seed) {
        AccTE<P> a = ld_te<P>(in);
        Niels28<P> n = ld_niels<P>(in + PTW);
        const Niels28<P> next = ld_niels<P>(in + PTW + NIW);
        te_madd_hot<P>(a, n, in[PTW + 2 * NIW] != 0, &next, in[PTW + 2 * NIW + 1] != 0, seed);
        st_te<P>(out, a); st_niels<P>(out + PTW, n);
    }
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) { run_seeded(in, out, FpMsm<P>::hot_loop_seed()); } };
// W products at once as te_madd_hot multiplies them: the zipped lower halves on the bias -1 (ff28.cuh mul_low_zip<X...>, X = the bound product of each operand pair),
// then the zipped upper halves.  in: a_0 b_0 a_1 b_1 ...; out: the W products
template <int... X> struct MulZip : OpBase { using G = Fp28<Fq377P>; static constexpr int W = sizeof...(X); static constexpr bool SEEDED = true;
    static constexpr int NIN = 2 * W * G::N, NOUT = W * G::N;
    ZK_HD static void run_seeded(const uint32_t *in, uint32_t *out, G::Seed seed) {
        G a[W], b[W], r[W];
        const G *pa[W], *pb[W];
        G *pr[W];
        typename G::Low lo[W];
        for (int w = 0; w < W; w++) { a[w] = ld<G>(in + 2 * w * G::N); b[w] = ld<G>(in + (2 * w + 1) * G::N); pa[w] = &a[w]; pb[w] = &b[w]; pr[w] = &r[w]; }
        const G *const (&cpa)[W] = pa; const G *const (&cpb)[W] = pb; G *const (&cpr)[W] = pr;
        G::template mul_low_zip<X...>(cpa, cpb, seed, lo);
        const typename G::Low (&clo)[W] = lo;
        G::template mul_high<W>(cpa, cpb, clo, cpr);
        for (int w = 0; w < W; w++) st<G>(out + w * G::N, r[w]);
    }
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) { run_seeded(in, out, G::hot_loop_seed()); } };
// in: accumulator, Affine28 (x, y); out: accumulator, then madd28's return value
template <class P> struct Madd28 : OpBase { static constexpr int NIN = PTW + 2 * GW, NOUT = PTW + 1;
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) {
        Acc28<P> a = ld_acc<P>(in);
        Affine28<P> q; q.x = ld<FpMsm<P>>(in + PTW); q.y = ld<FpMsm<P>>(in + PTW + GW);
        const bool ok = madd28<P>(a, q);
        st_acc<P>(out, a); out[PTW] = ok ? 1u : 0u;
    } };
template <class P> struct Add28 : OpBase { static constexpr int NIN = 2 * PTW, NOUT = PTW;
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) { Acc28<P> a = ld_acc<P>(in); add28<P>(a, ld_acc<P>(in + PTW)); st_acc<P>(out, a); } };
template <class P> struct Dbl28 : OpBase { static constexpr int NIN = PTW, NOUT = PTW;
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) { Acc28<P> a = ld_acc<P>(in); dbl28<P>(a); st_acc<P>(out, a); } };
template <class P> struct Neg28 : OpBase { static constexpr int NIN = PTW, NOUT = PTW;
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) { st_acc<P>(out, neg28<P>(ld_acc<P>(in))); } };
template <class P> struct ToStdPoint28 : OpBase { static constexpr int NIN = PTW, NOUT = 4 * P::N;
    ZK_HD static void run(const uint32_t *in, uint32_t *out, uint64_t) { st_xyzz<P>(out, to_std_point<P>(ld_acc<P>(in))); } };

// four lanes per case: lane q loads coordinate q of each operand and stores coordinate q of the result (kernels_msm.hip quad_load / quad_store)
struct TeAddQuad { using P = Fq377P; static constexpr bool QUAD = true; static constexpr int NIN = 2 * PTW, NOUT = PTW;
#if defined(__HIPCC__)
    __device__ __forceinline__ static void run_quad(const uint32_t *in, uint32_t *out, int q) { st(out + q * GW, te_add_quad<P>(ld<FpMsm<P>>(in + q * GW), ld<FpMsm<P>>(in + PTW + q * GW), q)); }
#endif
};
struct TeDblQuad { using P = Fq377P; static constexpr bool QUAD = true; static constexpr int NIN = PTW, NOUT = PTW;
#if defined(__HIPCC__)
    __device__ __forceinline__ static void run_quad(const uint32_t *in, uint32_t *out, int q) { st(out + q * GW, te_dbl_quad<P>(ld<FpMsm<P>>(in + q * GW), q)); }
#endif
};

// ---- the table.  Every template argument is one the kernels instantiate (sub<K>: ec28.cuh 2 3 4 5 7, te28.cuh 2 3 6; Fp29: kernels_ntt.hip, kernels_poly.hip).
#define ZK_PROBE_FP(X, B, F)                                                                                                                      \
    X(B + 0, Mul<F>) X(B + 1, Add<F>) X(B + 2, Sub<F>) X(B + 3, Neg<F>) X(B + 4, Dbl<F>) X(B + 5, Inverse<F>) X(B + 6, FromI64<F>) X(B + 7, PowU64<F>)       \
    X(B + 8, FromRaw<F>) X(B + 9, ToRaw<F>)
#define ZK_PROBE_FP28(X, B, P)                                                                                                                    \
    X(B + 0, Mul<Fp28<P>>) X(B + 1, Sqr<Fp28<P>>) X(B + 2, Fma2<Fp28<P>>) X(B + 3, Add<Fp28<P>>) X(B + 4, AddLazy<Fp28<P>>) X(B + 5, DblLazy<Fp28<P>>)          \
    X(B + 6, SubK<Fp28<P>, 2>) X(B + 7, SubK<Fp28<P>, 3>) X(B + 8, SubK<Fp28<P>, 4>) X(B + 9, SubK<Fp28<P>, 5>) X(B + 10, SubK<Fp28<P>, 6>) X(B + 11, SubK<Fp28<P>, 7>) \
    X(B + 12, SubLazyK<Fp28<P>, 2>) X(B + 13, SubLazyK<Fp28<P>, 3>) X(B + 14, Canonical<Fp28<P>>) X(B + 15, ProductIsZero<Fp28<P>>) X(B + 16, IsZeroModP<Fp28<P>>)   \
    X(B + 17, FromStd28<P>) X(B + 18, ToStd28<P>)
#define ZK_PROBE_FP29(X, B, P)                                                                                                                    \
    X(B + 0, Mul<Fp29<P>>) X(B + 1, Dot<Fp29<P>, 2>) X(B + 2, Dot<Fp29<P>, 3>) X(B + 3, Dot<Fp29<P>, 4>) X(B + 4, Add<Fp29<P>>) X(B + 5, AddLazy<Fp29<P>>)       \
    X(B + 6, SubK<Fp29<P>, 1>) X(B + 7, SubK<Fp29<P>, 2>) X(B + 8, SubK<Fp29<P>, 4>) X(B + 9, SubK<Fp29<P>, 8>) X(B + 10, SubLazyK<Fp29<P>, 2>)                \
    X(B + 11, Normalized<Fp29<P>>) X(B + 12, Shl5<Fp29<P>>) X(B + 13, CanonicalLog<Fp29<P>, 0>) X(B + 14, CanonicalLog<Fp29<P>, 1>) X(B + 15, CanonicalLog<Fp29<P>, 4>) \
    X(B + 16, ReduceTop<Fp29<P>>) X(B + 17, TwiddleFromStd<P>) X(B + 18, Split29<P>) X(B + 19, Pack29<P>)
#define ZK_PROBE_W28(X, B, P) X(B + 0, Madd28<P>) X(B + 1, Add28<P>) X(B + 2, Dbl28<P>) X(B + 3, Neg28<P>) X(B + 4, ToStdPoint28<P>)
#define ZK_PROBE_OPS(X)                                                                                                                           \
    ZK_PROBE_FP(X, 0, Fr377) ZK_PROBE_FP(X, 16, Fr381) ZK_PROBE_FP(X, 32, Fq377) ZK_PROBE_FP(X, 48, Fq381)                                         \
    ZK_PROBE_FP28(X, 64, Fq377P) X(64 + 19, MulBiased<Fp28<Fq377P>>) ZK_PROBE_FP28(X, 96, Fq381P)                                                  \
    ZK_PROBE_FP29(X, 128, Fr377P) ZK_PROBE_FP29(X, 160, Fr381P)                                                                                    \
    X(192, TeMadd) X(193, TeAdd) X(194, TeDbl) X(195, TeNeg) X(196, TeToStd) X(197, NielsFromW) X(198, TeMaddHot) X(199, TeAddQuad) X(200, TeDblQuad) \
    ZK_PROBE_W28(X, 208, Fq377P) ZK_PROBE_W28(X, 216, Fq381P)

// the zip probes, outside the table above (ids beyond MAX_OP_ID; api.py ARITH_ZIP_OPS names them): a lone product at the two bound products that differ in their
// switch-over column, and the two zips of te_madd_hot
#define ZK_PROBE_ZIP_OPS(X) X(232, MulZip<12>) X(233, MulZip<8>) X(234, MulZip<5, 2, 1>) X(235, MulZip<12, 8, 6, 12>)

template <class O> struct Tag { using type = O; };
// fn(Tag<Op>{}) for the operation with this id; false for an unknown id
template <class Fn> bool dispatch(int op, Fn &&fn) {
    switch (op) {
#define ZK_PROBE_CASE(ID, ...) case ID: fn(Tag<__VA_ARGS__>{}); return true;
        ZK_PROBE_OPS(ZK_PROBE_CASE)
#undef ZK_PROBE_CASE
        default: return false;
    }
}
template <class Fn> bool dispatch_zip(int op, Fn &&fn) {
    switch (op) {
#define ZK_PROBE_CASE(ID, ...) case ID: fn(Tag<__VA_ARGS__>{}); return true;
        ZK_PROBE_ZIP_OPS(ZK_PROBE_CASE)
#undef ZK_PROBE_CASE
        default: return false;
    }
}
constexpr int MAX_OP_ID = 224;
constexpr size_t MAX_CASES = (size_t)1 << 16;

}  // namespace probe
}  // namespace zk
