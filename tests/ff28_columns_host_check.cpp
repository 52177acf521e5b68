// tests/ff28_columns_host_check.cpp -- the Fp28 products of csrc/ff28.cuh (lower half row-wise, upper half carry-seeded column chains) against the exact integer
// (a b + M p) / R', M = -a b p^-1 mod R', R' = 2^392, computed here with plain big-integer arithmetic.  Stand-alone: own main, built by
// tests/test_ff28_columns_host.py with -fsanitize=address,undefined (the host branch of the header: no pins, the same terms in the same order).
//
// Every product (operator*, mul_biased, sqr, fma2, and the zipped mul_low / mul_high<W> pair te_madd_hot uses) must return that integer LIMB FOR LIMB -- normalized limbs,
// the excess in the top limb -- for normalized and for lazy operands alike, and a value below 1.2 p where the operands are inside the header's contract
// (limb products summing to at most 0.2 R' p: the criterion of tests/arith_model.py).
#include "ff28.cuh"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace zk;

// ---- non-negative integers of up to 2048 bits, little-endian 32-bit words; everything truncates at 2048 bits (the largest value here is below 2^800)
struct Big {
    static constexpr int W = 64;
    uint32_t w[W];
    Big() { memset(w, 0, sizeof w); }
    explicit Big(uint64_t v) : Big() { w[0] = (uint32_t)v; w[1] = (uint32_t)(v >> 32); }
    static Big from_limbs(const uint32_t *l, int n, int bits) {          // sum l_i 2^(bits i), limbs of up to 32 bits
        Big r;
        for (int i = 0; i < n; i++) {
            const int bit = bits * i, k = bit >> 5, sh = bit & 31;
            uint64_t v = (uint64_t)l[i] << sh, c = 0;
            for (int j = k; j < W && (v || c); j++) { const uint64_t s = (uint64_t)r.w[j] + (uint32_t)v + c; r.w[j] = (uint32_t)s; c = s >> 32; v >>= 32; }
        }
        return r;
    }
    Big operator+(const Big &b) const { Big r; uint64_t c = 0; for (int i = 0; i < W; i++) { const uint64_t s = (uint64_t)w[i] + b.w[i] + c; r.w[i] = (uint32_t)s; c = s >> 32; } return r; }
    Big operator-(const Big &b) const { Big r; int64_t c = 0; for (int i = 0; i < W; i++) { const int64_t s = (int64_t)w[i] - b.w[i] + c; r.w[i] = (uint32_t)s; c = s >> 32; } return r; }
    Big operator*(const Big &b) const {
        Big r;
        for (int i = 0; i < W; i++) {
            if (!w[i]) continue;
            uint64_t c = 0;
            for (int j = 0; i + j < W; j++) { const uint64_t s = (uint64_t)w[i] * b.w[j] + r.w[i + j] + c; r.w[i + j] = (uint32_t)s; c = s >> 32; }
        }
        return r;
    }
    Big low_bits(int bits) const { Big r; for (int i = 0; i < W; i++) { const int lo = 32 * i; r.w[i] = lo + 32 <= bits ? w[i] : (lo >= bits ? 0 : w[i] & ((1u << (bits - lo)) - 1)); } return r; }
    Big shr(int bits) const {
        Big r;
        const int k = bits >> 5, sh = bits & 31;
        for (int i = 0; i + k < W; i++) r.w[i] = sh ? (uint32_t)(((uint64_t)w[i + k] | ((uint64_t)(i + k + 1 < W ? w[i + k + 1] : 0) << 32)) >> sh) : w[i + k];
        return r;
    }
    bool is_zero() const { for (int i = 0; i < W; i++) if (w[i]) return false; return true; }
    int cmp(const Big &b) const { for (int i = W - 1; i >= 0; i--) if (w[i] != b.w[i]) return w[i] < b.w[i] ? -1 : 1; return 0; }
};

static uint64_t rng_state;
static uint64_t rnd64() { uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }

template <class P>
struct Check {
    using G = Fp28<P>;
    static constexpr int N = G::N, RBITS = 28 * G::N;
    Big p, pinv;                 // p^-1 mod R'
    int bad = 0, products = 0;

    Check() {
        uint32_t pl[N];
        for (int i = 0; i < N; i++) pl[i] = G::mod28(i);
        p = Big::from_limbs(pl, N, 28);
        Big x(1);                // Newton: x <- x (2 - p x) doubles the correct low bits (p is odd: 1 is right mod 2)
        for (int k = 0; k < 10; k++) x = (x * (Big(2) - (p * x).low_bits(RBITS)).low_bits(RBITS)).low_bits(RBITS);
        pinv = x;
        if ((p * pinv).low_bits(RBITS).cmp(Big(1)) != 0) { printf("p^-1 wrong\n"); bad++; }
    }
    static Big value(const G &a) { return Big::from_limbs(a.l, N, 28); }
    static G limbs(const Big &v) {                                       // normalized limbs of a value below 2^396 or so, the excess in the top limb
        G r;
        for (int i = 0; i < N - 1; i++) r.l[i] = v.shr(28 * i).w[0] & G::MASK;
        r.l[N - 1] = v.shr(28 * (N - 1)).w[0];
        return r;
    }
    // t: the sum of the limb products as an integer; got: what the routine returned
    void expect(const Big &t, const G &got, const char *what) {
        products++;
        const Big m = (Big() - (t * pinv).low_bits(RBITS)).low_bits(RBITS);          // -t p^-1 mod R'
        const Big s = t + m * p;
        if (!s.low_bits(RBITS).is_zero()) { printf("%s: model not exact\n", what); bad++; return; }
        const Big q = s.shr(RBITS);
        if (!q.shr(28 * (N - 1) + 32).is_zero()) { printf("%s: the top limb's excess does not fit\n", what); bad++; return; }
        const G want = limbs(q);
        for (int i = 0; i < N; i++)
            if (want.l[i] != got.l[i]) { printf("%s: limb %d is %08x, want %08x\n", what, i, got.l[i], want.l[i]); bad++; return; }
        // inside the contract (t <= 0.2 R' p): below 1.2 p
        Big five_t = t + t + t + t + t, rp;
        { uint32_t sh[N + 1] = {0}; sh[N] = 1; rp = Big::from_limbs(sh, N + 1, 28) * p; }          // R' p
        if (five_t.cmp(rp) <= 0) {
            Big ten_q = q + q; ten_q = ten_q + ten_q + q; ten_q = ten_q + ten_q;      // 10 q
            Big twelve_p = p + p + p; twelve_p = twelve_p + twelve_p; twelve_p = twelve_p + twelve_p;
            if (ten_q.cmp(twelve_p) >= 0) { printf("%s: product of operands inside the contract is not below 1.2 p\n", what); bad++; }
        }
    }
    void mul(const G &a, const G &b) {
        const Big t = value(a) * value(b);
        expect(t, a * b, "operator*");
        if constexpr (G::mod28(0) == 1u && G::PINV == G::MASK) {
            expect(t, G::mul_biased(a, b, G::hot_loop_bias()), "mul_biased");
        }
    }
    void sqr(const G &a) { expect(value(a) * value(a), a.sqr(), "sqr"); }
    void fma2(const G &a, const G &b, const G &c, const G &d) { expect(value(a) * value(b) + value(c) * value(d), G::fma2(a, b, c, d), "fma2"); }
    // the zipped form: W lower halves, then the W upper halves step by step
    template <int W> void zipped(const G (&a)[W], const G (&b)[W]) {
        if constexpr (G::mod28(0) == 1u && G::PINV == G::MASK) {
            typename G::Low lo[W];
            const G *pa[W], *pb[W];
            G r[W], *pr[W];
            for (int w = 0; w < W; w++) { lo[w] = G::mul_low(a[w], b[w], G::hot_loop_bias()); pa[w] = &a[w]; pb[w] = &b[w]; pr[w] = &r[w]; }
            const typename G::Low (&clo)[W] = lo;
            const G *const (&cpa)[W] = pa; const G *const (&cpb)[W] = pb; G *const (&cpr)[W] = pr;
            G::template mul_high<W>(cpa, cpb, clo, cpr);
            for (int w = 0; w < W; w++) expect(value(a[w]) * value(b[w]), r[w], "mul_low + mul_high<W>");
        }
    }
    static G all(uint32_t limb, uint32_t top) { G r; for (int i = 0; i < N; i++) r.l[i] = i == N - 1 ? top : limb; return r; }
    G random_below(int kp) {                                             // pseudo-random normalized limbs, value below kp x p
        const uint32_t top = (uint32_t)(((uint64_t)G::mod28(N - 1) * kp));
        G r;
        for (int i = 0; i < N - 1; i++) r.l[i] = (uint32_t)rnd64() & G::MASK;
        r.l[N - 1] = (uint32_t)(rnd64() % top);
        return r;
    }

    int run(const char *name, int kp_mul) {
        rng_state = 0x5eed;
        const Big one(1);
        // 0, 1, p - 1, p, 2 p re-limbed; all limbs MASK
        std::vector<G> sp = {limbs(Big()), limbs(one), limbs(p - one), limbs(p), limbs(p + p), all(G::MASK, G::MASK)};
        for (const G &a : sp) {
            sqr(a);
            for (const G &b : sp) {
                mul(a, b);
                fma2(a, b, b, a);
                fma2(a, b, sp[5], sp[5]);
            }
        }
        // the lazy extremes of te_madd_hot, EVERY limb (the top one too) at its bound: in units of 2^28, E < 3, H < 2, U < 4, V < 3.  The products the addition takes:
        // E F, G H, E H, F G with {F, G} = {U, V} -- the two widest are E U and U V (12 x 2^56 per limb product, 14 of them and 13 reduction products in a column)
        const uint32_t u28 = 1u << 28;
        const G E = all(3 * u28 - 1, 3 * u28 - 1), H = all(2 * u28 - 1, 2 * u28 - 1), U = all(4 * u28 - 1, 4 * u28 - 1), V = all(3 * u28 - 1, 3 * u28 - 1);
        const G hot_a[6] = {E, U, E, V, U, E}, hot_b[6] = {U, V, V, H, H, H};
        for (int i = 0; i < 6; i++) { mul(hot_a[i], hot_b[i]); mul(hot_b[i], hot_a[i]); }
        { const G a4[4] = {E, V, E, U}, b4[4] = {U, H, H, V}; zipped<4>(a4, b4); }           // one second level with neg = false: E F, G H, E H, F G
        { const G a4[4] = {E, U, E, V}, b4[4] = {V, H, H, U}; zipped<4>(a4, b4); }           // ... and with neg = true
        { const G a3[3] = {all(5 * u28 - 1, 1u << 20), H, sp[5]}, b3[3] = {sp[5], sp[5], sp[2]}; zipped<3>(a3, b3); }      // first level: sub_lazy<3> (limbs <= 5 x 2^28), add_lazy, T1
        // one step below each bound, and the bound in one limb position only
        for (int i = 0; i < N; i++) {
            G e = all(u28 - 1, 0), u = all(u28 - 1, 0);
            e.l[i] = 3 * u28 - 1; u.l[N - 1 - i] = 4 * u28 - 1;
            mul(e, u); mul(u, e);
        }
        // fma2 and sqr at their documented bounds: normalized limbs, all ones, and a top limb with twelve bits of excess beside it
        const G ones = all(G::MASK, G::MASK), big_top = all(G::MASK, (1u << 24) - 1);
        fma2(ones, ones, ones, ones);
        sqr(ones); sqr(big_top);
        for (const G &a : sp) { fma2(ones, a, a, ones); fma2(a, ones, ones, ones); }
        // 2,000 seeded random pairs (values below kp_mul x p: inside the product's contract), their squares, and two-product sums of values below 5 p
        for (int it = 0; it < 2000; it++) {
            const G a = random_below(kp_mul), b = random_below(kp_mul);
            mul(a, b);
            sqr(a);
            fma2(random_below(5), random_below(5), random_below(5), random_below(5));
            if (it < 200) { const G a3[3] = {a, b, a}, b3[3] = {b, b, a}; zipped<3>(a3, b3); }
        }
        printf("%s %d products %d bad\n", name, products, bad);
        return bad;
    }
};

int main() {
    // BLS12-377: inputs below 64 p; BLS12-381: a b < 500 p^2, e.g. both below 22 p (ff28.cuh)
    Check<Fq377P> c377;
    Check<Fq381P> c381;
    return (c377.run("fq377x28", 64) + c381.run("fq381x28", 22)) ? 1 : 0;
}
