// csrc/ff28.cuh -- reduced-radix ("lazy carry") Montgomery arithmetic for the 377/381-bit base fields on gfx950.
//
// Why: a 12x32-bit CIOS product compiles to 276 v_mad_u64_u32 + ~1000 full-rate fix-up instructions (64-bit adds and
// register-pair moves that only propagate carries); on MI355X v_mad_u64_u32 issues at ~0.4x the simple-VALU rate, so the
// fix-ups cost more than the multiplies (tools/ubench/rates.hip).  With 14 limbs of 28 bits a limb product is < 2^56 and a 64-bit
// accumulator absorbs all 28 products of a column, so the whole product is v_mad_u64_u32 with the accumulator as the addend:
// 2 * 14^2 = 392 multiply-accumulates and ~100 shifts/masks, no carry chain.
//
// Representation: value = sum l[i] 2^(28 i), limbs normalized to < 2^28 after every operation, Montgomery radix R' = 2^392.
// "Almost Montgomery": a product is < a b / R' + p, and R' / p is 2^15.3 (BLS12-377) / 2^11.3 (BLS12-381), so it is < 1.2 p and needs NO conditional subtraction for inputs
// < 64 p (377) or with a b < 500 p^2 (381: e.g. both < 22 p; the group law's operands stay below 8.2 p.  tests/arith_model.py asserts the bound per operand pair); additions and
// subtractions let values grow (sub adds a multiple of p) and callers bound them statically (see madd28 in kernels_msm.hip).
// Conversion from the library-wide 12x32 form (R = 2^384): split limbs, multiply by 2^8 R' mod p; back: multiply by R mod p... (to_std).
#pragma once
#include "ff.cuh"

namespace zk {

template <class P>   // P = Fq377P / Fq381P (12 x 32-bit parameter pack)
struct Fp28 {
    static constexpr int N = 14;
    static constexpr uint32_t MASK = (1u << 28) - 1;
    uint32_t l[N];

    // ---- constants derived at compile time from the 32-bit parameter pack
    ZK_HD static constexpr uint32_t mod28(int i) {           // limb i of p in radix 2^28
        int bit = 28 * i, w = bit >> 5, sh = bit & 31;
        uint64_t two = (w < P::N ? (uint64_t)P::mod(w) : 0) | ((w + 1 < P::N ? (uint64_t)P::mod(w + 1) : 0) << 32);
        return (uint32_t)(two >> sh) & MASK;
    }
    static constexpr uint32_t PINV = P::INV & MASK;   // -p^-1 mod 2^28 = the low 28 bits of -p^-1 mod 2^32

    ZK_HD static Fp28 zero() { Fp28 r; for (int i = 0; i < N; i++) r.l[i] = 0; return r; }
    ZK_HD bool limbs_zero() const { uint32_t o = 0; for (int i = 0; i < N; i++) o |= l[i]; return o == 0; }
    // v is a product (< 1.2 p): v == 0 (mod p)  <=>  v in {0, p}
    ZK_HD static bool product_is_zero(const Fp28 &v) {
        // one-limb pre-test first (hot path of k_accumulate: every VALU instruction counts): v in {0, p} needs limb 0 in {0, p_0}
        if (v.l[0] != 0u && v.l[0] != mod28(0)) return false;
        uint32_t z0 = 0, zp = 0;
#pragma unroll
        for (int i = 0; i < N; i++) { z0 |= v.l[i]; zp |= v.l[i] ^ mod28(i); }
        return z0 == 0 || zp == 0;
    }

    // split a 12x32 little-endian integer into 28-bit limbs (no arithmetic)
    ZK_HD static Fp28 split(const uint32_t *w) {
        Fp28 r;
#pragma unroll
        for (int i = 0; i < N; i++) {
            int bit = 28 * i, k = bit >> 5, sh = bit & 31;
            uint64_t two = (k < P::N ? (uint64_t)w[k] : 0) | ((k + 1 < P::N ? (uint64_t)w[k + 1] : 0) << 32);
            r.l[i] = (uint32_t)(two >> sh) & MASK;
        }
        return r;
    }
    // pack normalized limbs (value < 2^384) back into 12x32
    ZK_HD void pack(uint32_t *w) const {
#pragma unroll
        for (int k = 0; k < P::N; k++) {
            int bit = 32 * k, i = bit / 28, sh = bit % 28;     // word k = bits [32k, 32k+32)
            uint64_t v = (uint64_t)l[i] >> sh;
            int have = 28 - sh;
            if (i + 1 < N) v |= (uint64_t)l[i + 1] << have;
            if (have + 28 < 32 && i + 2 < N) v |= (uint64_t)l[i + 2] << (have + 28);
            w[k] = (uint32_t)v;
        }
    }
    // carry-propagate signed 64-bit limb values into normalized limbs (top limb keeps the excess)
    ZK_HD static Fp28 normalize(const int64_t *t) {
        Fp28 r;
        int64_t c = 0;
#pragma unroll
        for (int i = 0; i < N - 1; i++) { int64_t v = t[i] + c; r.l[i] = (uint32_t)v & MASK; c = v >> 28; }
        r.l[N - 1] = (uint32_t)(t[N - 1] + c);
        return r;
    }
    // a + b (no modular reduction; value grows)
    ZK_HD Fp28 operator+(const Fp28 &b) const {
        Fp28 r;
        uint32_t c = 0;
#pragma unroll
        for (int i = 0; i < N - 1; i++) { uint32_t v = l[i] + b.l[i] + c; r.l[i] = v & MASK; c = v >> 28; }
        r.l[N - 1] = l[N - 1] + b.l[N - 1] + c;
        return r;
    }
    ZK_HD Fp28 dbl() const { return *this + *this; }
    // ---- lazy limb arithmetic: NO carry propagation, limbs may exceed 28 bits.  Valid as ONE operand of a product whose other operand is normalized:
    // a column then holds at most 14 limb products of (2^30.4 x 2^28) plus the reduction's 14 x 2^56, below 2^63; two lazy operands only where the caller bounds
    // 14 x (limb bound a) x (limb bound b) + 14 x 2^56 below 2^64 (te28.cuh lists the operands that use it, with their bounds).
    ZK_HD Fp28 add_lazy(const Fp28 &b) const { Fp28 r; for (int i = 0; i < N; i++) r.l[i] = l[i] + b.l[i]; return r; }
    ZK_HD Fp28 dbl_lazy() const { Fp28 r; for (int i = 0; i < N; i++) r.l[i] = l[i] << 1; return r; }
    // b normalized; limbs <= (K + 2) 2^28.  On the device limbs 0..12 are ONE instruction each: kp_spread >= 2^28 - 1 >= b_i there, so l + (kp - b) = |kp - b| + l = v_sad_u32
    // (the top limb keeps the two-instruction form: b's excess sits there)
    template <int K> ZK_HD Fp28 sub_lazy(const Fp28 &b) const {
        Fp28 r;
#pragma unroll
        for (int i = 0; i < N; i++) {
#if defined(__HIP_DEVICE_COMPILE__)
            if (i < N - 1) { asm("v_sad_u32 %0, %1, %2, %3" : "=v"(r.l[i]) : "s"(kp_spread<K>(i)), "v"(b.l[i]), "v"(l[i])); continue; }
#endif
            r.l[i] = l[i] + kp_spread<K>(i) - b.l[i];
        }
        return r;
    }
    // limb i of K p (normalized; the top limb keeps the excess) and the same with the borrows pre-distributed:
    // sum c_i 2^(28 i) = K p with c_i >= 2^28 - 1 below the top, so a_i - b_i + c_i never goes negative for a normalized b
    template <int K> ZK_HD static constexpr uint32_t kp_limb(int i) {
        uint64_t c = 0, v = 0;
        for (int j = 0; j <= i; j++) { v = (uint64_t)K * mod28(j) + c; c = v >> 28; }
        return i == N - 1 ? (uint32_t)v : (uint32_t)v & MASK;
    }
    template <int K> ZK_HD static constexpr uint32_t kp_spread(int i) {
        return i == 0 ? kp_limb<K>(0) + (1u << 28) : (i == N - 1 ? kp_limb<K>(i) - 1u : kp_limb<K>(i) + MASK);
    }
    // a - b + K p, K chosen by the caller so that K p >= b (keeps the result non-negative); 32-bit unsigned arithmetic only, no borrow chain
    template <int K>
    ZK_HD Fp28 sub(const Fp28 &b) const {
        Fp28 r;
        uint32_t c = 0;
#pragma unroll
        for (int i = 0; i < N - 1; i++) { uint32_t v = l[i] + kp_spread<K>(i) - b.l[i] + c; r.l[i] = v & MASK; c = v >> 28; }
        r.l[N - 1] = l[N - 1] + kp_spread<K>(N - 1) - b.l[N - 1] + c;
        return r;
    }

    // one row of the Montgomery reduction: make limb i of t a multiple of 2^28 by adding m p, then carry it into limb i + 1.
    // For p = 1 (mod 2^28) (BLS12-377's q: -p^-1 = -1, limb 0 of p = 1) m = -t_i mod 2^28 and the low limb needs no multiply and no
    // 64-bit add of m: t_i + m clears the low 28 bits and carries exactly one unit when they were non-zero, i.e. (t_i + 2^28 - 1) >> 28.
    ZK_HD static void reduce_row(uint64_t *t, int i) {
        if constexpr (mod28(0) == 1u && PINV == MASK) {
            // u = t_i + 2^28 - 1: its high part is the carry (t_i + m) >> 28 (one unit exactly when the low 28 bits of t_i are non-zero) and its low 28 bits are
            // those of t_i - 1, so m = -t_i mod 2^28 = ~u mod 2^28
            const uint64_t u = t[i] + MASK;
            const uint32_t m = ~(uint32_t)u & MASK;
#pragma unroll
            for (int j = 1; j < N; j++) t[i + j] += (uint64_t)m * mod28(j);
            t[i + 1] += u >> 28;
        } else {
            uint32_t m = (((uint32_t)t[i] & MASK) * PINV) & MASK;
#pragma unroll
            for (int j = 0; j < N; j++) t[i + j] += (uint64_t)m * mod28(j);
            t[i + 1] += t[i] >> 28;
        }
    }

    // almost-Montgomery product: row-wise operand scanning, 64-bit column accumulators, no carry chain
    ZK_HD Fp28 operator*(const Fp28 &b) const {
        uint64_t t[2 * N];
#pragma unroll
        for (int i = 0; i < 2 * N; i++) t[i] = 0;
#pragma unroll
        for (int i = 0; i < N; i++) {
#pragma unroll
            for (int j = 0; j < N; j++) t[i + j] += (uint64_t)l[j] * b.l[i];
            reduce_row(t, i);
        }
        Fp28 r;
        uint64_t c = 0;
#pragma unroll
        for (int i = 0; i < N - 1; i++) { uint64_t v = t[N + i] + c; r.l[i] = (uint32_t)v & MASK; c = v >> 28; }
        r.l[N - 1] = (uint32_t)(t[2 * N - 1] + c);
        return r;
    }

    // ---- the hot loop's product, in two halves (p = 1 (mod 2^28) only: BLS12-377's q).  The row-wise form above sums every column first and joins the carries afterwards:
    // 27 stand-alone 64-bit adds (v_lshl_add_u64) per product, 14 row carries and 13 limb normalisations.
    // LOWER half (mul_low: columns 0..N-1, row-wise as above, restricted to the columns i + j < N): it leaves the N multipliers m_i and the carry out of column N - 1.
    // UPPER half (mul_high: columns N..2N-2, product scanning): a column's multiply-add chain STARTS from the carry of the column below -- v_mad_u64_u32 has a 64-bit
    // addend slot, so joining the carry costs nothing and the 13 normalisation adds go away.  (mul_low keeps the row-wise order: on ITS bias, 2^28 - 1, a row seeded with the
    // carry would cost the same shift, add of the bias and v_bitop3 it costs now; mul_low_zip below seeds the lower columns on the bias -1, where it does pay.)  LLVM re-associates a late-defined addend to the END of a sum, so on the device every step of a chain
    // is followed by an empty asm that pins the order; the host branch has none and adds the same terms in the same order.
    // Bound: a chain adds the non-negative terms of the row-wise form's column k and the carry that column was joined with, in another order; every partial sum is at most
    // that total, which is below 2^64 for every operand pair the callers document (normalized x lazy: < 2^63; te_madd_hot's lazy pairs: 181 x 2^56, te28.cuh).  Each
    // column yields the same limb and the same carry as the row-wise form: the result is the same integer limb for limb, not merely the same residue.
    // Price: a chain is a run of dependent v_mad_u64_u32, and gfx950 wants one wait state between a v_mad_u64_u32 and the one that reads its result.  A lone product
    // (W = 1) gets an s_nop wherever the compiler finds no independent instruction; te_madd_hot therefore ZIPS the products of one level (W = 3, W = 4): the chains advance
    // in turn, the pins are volatile -- which holds them, and with them the steps, in source order -- and a scheduling barrier at the entry keeps the lower halves (28
    // column registers each) from sinking into the zip, where they would overlap the W x 13 live multipliers.  k_accumulate<EdwardsLaw>: 188 -> 97 v_lshl_add_u64,
    // 3,495 -> 3,404 VALU, 7 s_nop in the loop, 165 registers (profiles/fq_product_carry_seed.md); with the lower half zipped as well (mul_low_zip) 21 v_lshl_add_u64,
    // 3,327 VALU, 23 s_nop, 166 registers (profiles/fq_product_lower_seed.md).
    // operator*, fma2 and sqr stay row-wise: their callers (bucket reduction, class sums, conversions) run them one at a time, the chains fill with s_nop (k_reduce_l1_pair:
    // 1,484; k_class_partials: 1,160) and with the upper half carry-seeded k_class_partials measured 12 % and k_quad_sum 5 % SLOWER, the reduction kernels no faster (same file).
    struct Low { uint32_t m[N]; uint64_t carry; };
    template <bool ZIPPED> ZK_HD static void pin(uint64_t &acc) {
#if defined(__HIP_DEVICE_COMPILE__)
        if constexpr (ZIPPED) asm volatile("" : "+v"(acc)); else asm("" : "+v"(acc));
#else
        (void)acc;
#endif
    }
    // columns start at `bias` = 2^28 - 1 (see mul_biased): when row i is reached, u = column i + 2^28 - 1, its high part is the row's carry and m_i = ~u mod 2^28 (reduce_row)
    ZK_HD static Low mul_low(const Fp28 &a, const Fp28 &b, uint64_t bias) {
        static_assert(mod28(0) == 1u && PINV == MASK, "written for p = 1 (mod 2^28)");
        uint64_t t[N];
        Low lo;
#pragma unroll
        for (int i = 0; i < N; i++) t[i] = bias;
#pragma unroll
        for (int i = 0; i < N; i++) {
#pragma unroll
            for (int j = 0; i + j < N; j++) t[i + j] += (uint64_t)a.l[j] * b.l[i];
            const uint64_t u = t[i];
            lo.m[i] = ~(uint32_t)u & MASK;
#pragma unroll
            for (int j = 1; i + j < N; j++) t[i + j] += (uint64_t)lo.m[i] * mod28(j);
            if (i + 1 < N) t[i + 1] += u >> 28; else lo.carry = u >> 28;
        }
        return lo;
    }
    // ---- the lower half as product scanning too, on a bias of -1 (te_madd_hot's seven products; p = 1 (mod 2^28) only).  A column is held as u' = t - 1, t its true value
    // with the carry from below:  ~u' mod 2^28 = -t mod 2^28 is the same multiplier m as above, and the carry into the next column, ceil(t / 2^28) = floor((t - 1) / 2^28) + 1,
    // is (u' >> 28, ARITHMETIC) + 1 -- so the next column's own "- 1" cancels the "+ 1" and the shift result IS the seed of the next column's multiply-add chain: one
    // v_bitop3_b32 and one v_ashrrev_i64 per column, no 64-bit add (the bias 2^28 - 1 of mul_low needs its "+ 2^28 - 1" again in every column, which rides free on a chain's
    // first addend only while the carry is joined by a separate add; -1 is the only bias that reproduces itself).  t = 0 (te_identity's all-zero x and t) gives u' = -1,
    // m = 0 and the seed -1 = the true carry 0, less one.  Column k's chain: the seed, the k + 1 terms a_(k-i) b_i, the k terms m_i p_(k-i) with m_(k-1) p_1 last.
    // Range: the arithmetic shift needs u' < 2^63 = 128 x 2^56.  With X the product of the two operands' limb bounds in units of 2^28, column k holds less than
    // ((k + 1) X + k + 1) x 2^56 (the a b terms, the m p terms, a carry below 2^36); signed_columns(X) is the number of columns, from column 0 up, for which that stays at or
    // below 128 -- all 14 for X <= 8, nine for X = 12.  The columns above switch to mul_low's unsigned form: the first of them adds 2^28 to its seed (from the bias -1 to
    // the bias 2^28 - 1), the later ones are seeded with (u >> 28, logical) + 2^28 - 1, and the carry out of column 13 is then the true carry; a product that stays signed
    // to the end adds 1 once, where it hands its carry to mul_high.  Both bounds are static assertions on X: wider operands do not compile.
    // `seed` must hold -1 in a register pair the compiler cannot see through, defined before the operands (hot_loop_seed() at kernel entry), for the reason `bias` must.
    // The same m_i enter the same columns as in mul_low: lo is the same, and with it the product, limb for limb.  Chains of dependent v_mad_u64_u32 again: the W products
    // are zipped, pins volatile, a scheduling barrier at the entry (see mul_high).
    struct Seed { uint64_t v; };                                   // a type of its own: the row-wise bias 2^28 - 1 must not be passed for it
    ZK_HD static constexpr int signed_columns(int x) { int k = 0; while (k < N && (k + 1) * x + k + 1 <= 128) k++; return k; }
    template <int... X>
    ZK_HD static void mul_low_zip(const Fp28 *const (&a)[sizeof...(X)], const Fp28 *const (&b)[sizeof...(X)], Seed seed, Low (&lo)[sizeof...(X)]) {
        static_assert(mod28(0) == 1u && PINV == MASK, "written for p = 1 (mod 2^28)");
        constexpr int W = sizeof...(X);
        constexpr int SW[W] = {signed_columns(X)...};
        static_assert(((X >= 1 && signed_columns(X) >= 1 && N * X + N <= 256) && ...), "operand limb bounds too wide for the 64-bit columns");
        uint64_t acc[W];
#if defined(__HIP_DEVICE_COMPILE__)
        if constexpr (W > 1) __builtin_amdgcn_sched_barrier(0);
#endif
#pragma unroll
        for (int w = 0; w < W; w++) acc[w] = seed.v;
#pragma unroll
        for (int k = 0; k < N; k++) {
#pragma unroll
            for (int i = 0; i <= k; i++) {
#pragma unroll
                for (int w = 0; w < W; w++) { acc[w] += (uint64_t)a[w]->l[k - i] * b[w]->l[i]; pin<(W > 1)>(acc[w]); }
            }
#pragma unroll
            for (int i = 0; i < k; i++) {
#pragma unroll
                for (int w = 0; w < W; w++) { acc[w] += (uint64_t)lo[w].m[i] * mod28(k - i); pin<(W > 1)>(acc[w]); }
            }
#pragma unroll
            for (int w = 0; w < W; w++) {
                const uint64_t u = acc[w];
                lo[w].m[k] = ~(uint32_t)u & MASK;
                uint64_t next;
                if (k < SW[w]) {                                   // u = t - 1: the seed of the next column, which is the true carry less one
                    next = (uint64_t)((int64_t)u >> 28);
                    if (k + 1 == N) next += 1;
                    else if (k + 1 == SW[w]) next += (uint64_t)MASK + 1;
                } else {                                           // u = t + 2^28 - 1: the true carry
                    next = u >> 28;
                    if (k + 1 < N) next += MASK;
                }
                if (k + 1 < N) acc[w] = next; else lo[w].carry = next;
            }
        }
    }
    ZK_HD static Seed hot_loop_seed() {
        uint64_t v = ~(uint64_t)0;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+s"(v));
#endif
        return Seed{v};
    }
    // the upper halves of the W independent products a[w] b[w] whose lower halves are lo[w], zipped step by step; r[w] must not alias an operand
    template <int W>
    ZK_HD static void mul_high(const Fp28 *const (&a)[W], const Fp28 *const (&b)[W], const Low (&lo)[W], Fp28 *const (&r)[W]) {
        uint64_t carry[W];
#if defined(__HIP_DEVICE_COMPILE__)
        if constexpr (W > 1) __builtin_amdgcn_sched_barrier(0);
#endif
#pragma unroll
        for (int w = 0; w < W; w++) carry[w] = lo[w].carry;
#pragma unroll
        for (int k = N; k < 2 * N - 1; k++) {
            uint64_t acc[W];
#pragma unroll
            for (int w = 0; w < W; w++) acc[w] = carry[w];
#pragma unroll
            for (int i = k - N + 1; i < N; i++) {
#pragma unroll
                for (int w = 0; w < W; w++) {
                    acc[w] += (uint64_t)a[w]->l[k - i] * b[w]->l[i]; pin<(W > 1)>(acc[w]);
                    acc[w] += (uint64_t)lo[w].m[i] * mod28(k - i); pin<(W > 1)>(acc[w]);
                }
            }
#pragma unroll
            for (int w = 0; w < W; w++) { r[w]->l[k - N] = (uint32_t)acc[w] & MASK; carry[w] = acc[w] >> 28; }
        }
#pragma unroll
        for (int w = 0; w < W; w++) r[w]->l[N - 1] = (uint32_t)carry[w];       // column 2N - 1 holds nothing but the last carry: the top limb keeps the excess
    }
    // The same product as operator* in the two halves above (mul_low, mul_high<1>), with the rows' "+ 2^28 - 1" riding on the multiply-accumulate chains: columns 0..13
    // START at `bias`, which must hold 2^28 - 1 in a register pair the compiler cannot see through and that was defined before the operands (hot_loop_bias() at kernel
    // entry).  A known constant is re-associated to the end of every column's sum and costs a 64-bit add per row -- 14 per product; an unknown early value stays the
    // chain's first addend.
    ZK_HD static Fp28 mul_biased(const Fp28 &a, const Fp28 &b, uint64_t bias) {
        Fp28 r;
        const Low lo[1] = {mul_low(a, b, bias)};
        const Fp28 *const pa[1] = {&a}, *const pb[1] = {&b};
        Fp28 *const pr[1] = {&r};
        mul_high<1>(pa, pb, lo, pr);
        return r;
    }
    ZK_HD static uint64_t hot_loop_bias() {
        uint64_t v = MASK;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+s"(v));
#endif
        return v;
    }
    // (a b + c d) / R' with ONE Montgomery reduction: both limb products accumulate into the same 64-bit columns (28 products of < 2^56
    // plus the 14 reduction products per column stay below 2^62), which saves the 196 multiplies of a second reduction.
    // Inputs normalized; the result is < ((a b + c d) / R') + p, e.g. < 1.01 p for a b + c d < 64 p^2.
    ZK_HD static Fp28 fma2(const Fp28 &a, const Fp28 &b, const Fp28 &c, const Fp28 &d) {
        uint64_t t[2 * N];
#pragma unroll
        for (int i = 0; i < 2 * N; i++) t[i] = 0;
#pragma unroll
        for (int i = 0; i < N; i++) {
#pragma unroll
            for (int j = 0; j < N; j++) t[i + j] += (uint64_t)a.l[j] * b.l[i];
#pragma unroll
            for (int j = 0; j < N; j++) t[i + j] += (uint64_t)c.l[j] * d.l[i];
            reduce_row(t, i);
        }
        Fp28 r;
        uint64_t cy = 0;
#pragma unroll
        for (int i = 0; i < N - 1; i++) { uint64_t v = t[N + i] + cy; r.l[i] = (uint32_t)v & MASK; cy = v >> 28; }
        r.l[N - 1] = (uint32_t)(t[2 * N - 1] + cy);
        return r;
    }
    // squaring: the 105 distinct limb products (cross terms doubled by pre-doubling one operand) instead of 196; same reduction
    ZK_HD Fp28 sqr() const {
        uint64_t t[2 * N];
#pragma unroll
        for (int i = 0; i < 2 * N; i++) t[i] = 0;
        uint32_t d[N];
#pragma unroll
        for (int i = 0; i < N; i++) d[i] = l[i] << 1;                      // < 2^29 (top limb of a bounded value stays far below 2^31)
#pragma unroll
        for (int i = 0; i < N; i++) {
            t[2 * i] += (uint64_t)l[i] * l[i];
#pragma unroll
            for (int j = i + 1; j < N; j++) t[i + j] += (uint64_t)d[i] * l[j];
        }
#pragma unroll
        for (int i = 0; i < N; i++) {
            reduce_row(t, i);
        }
        Fp28 r;
        uint64_t c = 0;
#pragma unroll
        for (int i = 0; i < N - 1; i++) { uint64_t v = t[N + i] + c; r.l[i] = (uint32_t)v & MASK; c = v >> 28; }
        r.l[N - 1] = (uint32_t)(t[2 * N - 1] + c);
        return r;
    }

    // fully reduce a value < 64 p to the canonical range [0, p) (used only at conversions and for zero tests)
    ZK_HD Fp28 canonical() const {
        Fp28 v = *this;
        // subtract p while v >= p: at most 64 rounds would be wasteful; peel powers of two: 32p, 16p, ... p
#pragma unroll
        for (int k = 5; k >= 0; k--) {
            // t = v - (2^k) p
            int64_t c = 0;
            uint32_t tl[N];
#pragma unroll
            for (int i = 0; i < N - 1; i++) { int64_t x = (int64_t)v.l[i] - ((int64_t)mod28(i) << k) + c; tl[i] = (uint32_t)x & MASK; c = x >> 28; }
            int64_t top = (int64_t)v.l[N - 1] - ((int64_t)mod28(N - 1) << k) + c;
            if (top >= 0) {
#pragma unroll
                for (int i = 0; i < N - 1; i++) v.l[i] = tl[i];
                v.l[N - 1] = (uint32_t)top;
            }
        }
        return v;
    }
    ZK_HD bool is_zero_mod_p() const { return canonical().limbs_zero(); }

    // constants: 2^8 R' mod p ... obtained at run time from the 32-bit field (host + device) to avoid a second generated table
    ZK_HD static Fp28 from_std(const Fp<P> &a) {
        // a = x R (R = 2^384).  want x R' (R' = 2^392) = a 2^8.  mul28(split(a), c) = a c / R'  with c = 2^8 R'^1 ... = 2^400 mod p
        Fp28 s = split(a.l);
        return s * k_2_400();
    }
    ZK_HD Fp<P> to_std() const {
        // w = x R'.  mul28(w, 2^384 mod p) = x 2^384 = standard Montgomery form; then canonicalize and repack
        Fp28 y = (*this * k_2_384()).canonical();
        Fp<P> r;
        y.pack(r.l);
        return r;
    }
    // 2^400 mod p and 2^384 mod p as 28-bit limb integers, computed from Fp<P> (R = 2^384: one() = 2^384 mod p)
    ZK_HD static Fp28 k_2_384() { Fp<P> o = Fp<P>::one(); return split(o.l); }
    ZK_HD static Fp28 k_one() { return k_2_392(); }
    ZK_HD static Fp28 k_2_392() {               // the Montgomery one of this representation (R' mod p)
        Fp<P> v = Fp<P>::one();
        for (int i = 0; i < 8; i++) v = v.dbl();
        return split(v.l);
    }
    ZK_HD static Fp28 k_2_400() {
        // 2^400 mod p = (2^384 mod p) * 2^16 mod p : in Montgomery form of Fp<P>: from_u64(2^16) * one ... compute raw integer:
        Fp<P> v = Fp<P>::one();                 // raw limbs = 2^384 mod p  (as an integer)
        for (int i = 0; i < 16; i++) v = v.dbl();   // integer doubling mod p of the raw limbs (Fp add is plain modular add on the limbs)
        return split(v.l);
    }
};

using Fq377x28 = Fp28<Fq377P>;
using Fq381x28 = Fp28<Fq381P>;

}  // namespace zk
