// tests/ff28_lower_seed_host_check.cpp -- the Fq377 product with its LOWER half carry-seeded on a bias of -1 (csrc/ff28.cuh mul_low_zip<X...> followed by mul_high<W>,
// W = 1, 3, 4) against exact integer Montgomery reduction, limb for limb.  Stand-alone: own main, built by tests/test_ff28_lower_seed_host.py with
// -fsanitize=address,undefined (the host branch of the header: no pins, the same terms in the same order, the sums in uint64_t).
//
// The reference keeps the 28 columns of a b in 128-bit integers (a column is below 2^70: nothing wraps), reduces row by row with m_i = -t_i mod 2^28 -- the digits of the
// one M = -a b p^-1 mod R' -- and propagates every carry: (a b + M p) / R' as an integer, normalized limbs, the excess in the top limb.
// Beside the product it checks, with the multipliers the header returned, what the header's static assertions promise: in every column that takes the arithmetic shift
// u' = t - 1 lies in [-1, 2^63), in every column above t + 2^28 - 1 is below 2^64; and that at the bound of the two wide products a column above the switch-over does
// exceed 2^63 -- the fallback columns are needed, and they run.
#include "ff28.cuh"
#include <cstdio>
#include <vector>
using namespace zk;

using G = Fp28<Fq377P>;
using u128 = unsigned __int128;
using i128 = __int128;
constexpr int N = G::N;
constexpr uint32_t U28 = 1u << 28;

static uint64_t rng_state = 0x10e5eed;
static uint64_t rnd64() { uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }

static int bad = 0, products = 0, signed_columns_seen = 0, fallback_columns_seen = 0, fallback_needed = 0, zero_columns_seen = 0;

struct Ref { G r; uint32_t m[N]; u128 t[N]; };          // the product, the multipliers, and the true value of every lower column (carry from below included)
static Ref reference(const G &a, const G &b) {
    u128 t[2 * N] = {0};
    for (int i = 0; i < N; i++) for (int j = 0; j < N; j++) t[i + j] += (u128)a.l[j] * b.l[i];
    Ref o;
    for (int i = 0; i < N; i++) {
        o.t[i] = t[i];
        const uint32_t m = (uint32_t)((U28 - (uint32_t)(t[i] & G::MASK)) & G::MASK);
        o.m[i] = m;
        for (int j = 0; j < N; j++) t[i + j] += (u128)m * G::mod28(j);
        if ((uint32_t)(t[i] & G::MASK)) { printf("reference: row %d not cleared\n", i); bad++; }
        t[i + 1] += t[i] >> 28;
    }
    for (int i = 0; i < N - 1; i++) { o.r.l[i] = (uint32_t)(t[N + i] & G::MASK); t[N + i + 1] += t[N + i] >> 28; }
    if (t[2 * N - 1] >> 32) { printf("reference: the top limb's excess does not fit\n"); bad++; }
    o.r.l[N - 1] = (uint32_t)t[2 * N - 1];
    return o;
}

// one product of a zip: result, multipliers, carry and the column ranges; X = the bound product the zip was instantiated with; at_bound: every limb of both operands at its bound
static void expect(const G &a, const G &b, const G &got, const G::Low &lo, int X, bool at_bound, const char *what) {
    products++;
    const Ref want = reference(a, b);
    for (int i = 0; i < N; i++)
        if (want.r.l[i] != got.l[i]) { printf("%s (X = %d): limb %d is %08x, want %08x\n", what, X, i, got.l[i], want.r.l[i]); bad++; return; }
    for (int i = 0; i < N; i++)
        if (want.m[i] != lo.m[i]) { printf("%s (X = %d): multiplier %d is %07x, want %07x\n", what, X, i, lo.m[i], want.m[i]); bad++; return; }
    const u128 carry = (want.t[N - 1] + want.m[N - 1]) >> 28;
    if ((u128)lo.carry != carry) { printf("%s (X = %d): the carry into column %d is not the true carry\n", what, X, N); bad++; return; }
    const int sw = G::signed_columns(X);
    bool over = false;
    for (int k = 0; k < N; k++) {
        const i128 u = (i128)want.t[k] - 1;                                  // what a signed column holds
        if (k < sw) {
            signed_columns_seen++;
            if (want.t[k] == 0) zero_columns_seen++;
            if (u < -1 || u >= ((i128)1 << 63)) { printf("%s (X = %d): column %d leaves the signed range\n", what, X, k); bad++; return; }
        } else {
            fallback_columns_seen++;
            if (u >= ((i128)1 << 63)) over = true;
            if (want.t[k] + G::MASK >= ((u128)1 << 64)) { printf("%s (X = %d): column %d leaves the unsigned range\n", what, X, k); bad++; return; }
        }
    }
    if (over) fallback_needed++;
    if (at_bound && sw < N && !over) { printf("%s (X = %d): at the bound no fallback column exceeds 2^63 -- the switch-over is not exercised\n", what, X); bad++; }
    // the row-wise lower half leaves the same multipliers and the same carry wherever its unsigned columns hold the operands
    const G::Low row = G::mul_low(a, b, G::hot_loop_bias());
    for (int i = 0; i < N; i++) if (row.m[i] != lo.m[i]) { printf("%s (X = %d): multiplier %d differs from mul_low's\n", what, X, i); bad++; return; }
    if (row.carry != lo.carry) { printf("%s (X = %d): carry differs from mul_low's\n", what, X); bad++; }
}

template <int... X> static void zip(const G (&a)[sizeof...(X)], const G (&b)[sizeof...(X)], bool at_bound, const char *what) {
    constexpr int W = sizeof...(X);
    constexpr int xs[W] = {X...};
    G::Low lo[W];
    const G *pa[W], *pb[W];
    G r[W], *pr[W];
    for (int w = 0; w < W; w++) { pa[w] = &a[w]; pb[w] = &b[w]; pr[w] = &r[w]; }
    const G *const (&cpa)[W] = pa; const G *const (&cpb)[W] = pb; G *const (&cpr)[W] = pr;
    G::template mul_low_zip<X...>(cpa, cpb, G::hot_loop_seed(), lo);
    const G::Low (&clo)[W] = lo;
    G::template mul_high<W>(cpa, cpb, clo, cpr);
    for (int w = 0; w < W; w++) expect(a[w], b[w], r[w], lo[w], xs[w], at_bound, what);
}

static G all(uint32_t limb) { G r; for (int i = 0; i < N; i++) r.l[i] = limb; return r; }
static G random_below(int x) { G r; for (int i = 0; i < N; i++) r.l[i] = (uint32_t)(rnd64() % ((uint64_t)x * U28)); return r; }
static G edges(int x) {                                                       // limbs from {0, 1, bound - 1, random}
    G r;
    for (int i = 0; i < N; i++) {
        const uint64_t c = rnd64();
        r.l[i] = (c & 3) == 0 ? 0u : (c & 3) == 1 ? 1u : (c & 3) == 2 ? (uint32_t)x * U28 - 1 : (uint32_t)((c >> 8) % ((uint64_t)x * U28));
    }
    return r;
}
static G low_zero(int x) { G r = random_below(x); r.l[0] = 0; return r; }

// the operand lists for one pair of limb bounds (xa, xb, in units of 2^28) in a product slot instantiated for the bound product X >= xa xb
template <int X> static void pair_cases(int xa, int xb, int randoms) {
    std::vector<G> as, bs;
    std::vector<bool> bound;
    auto add = [&](const G &a, const G &b, bool at = false) { as.push_back(a); bs.push_back(b); bound.push_back(at); };
    const G za = all(0), ba = all((uint32_t)xa * U28 - 1), bb = all((uint32_t)xb * U28 - 1);
    add(ba, bb, xa * xb == X);                                                 // every limb at its bound
    add(za, bb); add(ba, za); add(za, za);                                     // an all-zero operand on either side: every column is t = 0, u' = -1
    add(za, random_below(xb)); add(random_below(xa), za);
    for (int i = 0; i < 8; i++) { add(low_zero(xa), random_below(xb)); add(random_below(xa), low_zero(xb)); add(low_zero(xa), low_zero(xb)); }
    for (int i = 0; i < 400; i++) add(edges(xa), edges(xb));
    for (int i = 0; i < randoms; i++) add(random_below(xa), random_below(xb));
    while (as.size() % 12) add(random_below(xa), random_below(xb));
    for (size_t i = 0; i < as.size(); i++) {                                   // alone ...
        const G a1[1] = {as[i]}, b1[1] = {bs[i]};
        zip<X>(a1, b1, bound[i], "mul_low_zip<X> + mul_high<1>");
    }
    for (size_t i = 0; i + 3 <= as.size(); i += 3) {                           // ... three wide ...
        const G a3[3] = {as[i], as[i + 1], as[i + 2]}, b3[3] = {bs[i], bs[i + 1], bs[i + 2]};
        zip<X, X, X>(a3, b3, false, "mul_low_zip<X, X, X> + mul_high<3>");
    }
    for (size_t i = 0; i + 4 <= as.size(); i += 4) {                           // ... and four wide
        const G a4[4] = {as[i], as[i + 1], as[i + 2], as[i + 3]}, b4[4] = {bs[i], bs[i + 1], bs[i + 2], bs[i + 3]};
        zip<X, X, X, X>(a4, b4, false, "mul_low_zip<X, X, X, X> + mul_high<4>");
    }
}

int main() {
    static_assert(G::signed_columns(1) == 14 && G::signed_columns(5) == 14 && G::signed_columns(6) == 14 && G::signed_columns(8) == 14 && G::signed_columns(12) == 9,
                  "the switch-over columns te_madd_hot is documented with");
    // the seven operand pairs of te_madd_hot, in units of 2^28: (Y - X + 3p') n < 5 x 1, (Y + X) n < 2 x 1, T n < 1 x 1; E < 3, H < 2, U < 4, V < 3 with
    // E F in {E U, E V}, G H in {U H, V H}, E H, F G = U V (either order) -- each in the slot (X) te_madd_hot instantiates for it
    pair_cases<5>(5, 1, 3000); pair_cases<2>(2, 1, 3000); pair_cases<1>(1, 1, 3000);
    pair_cases<12>(3, 4, 3000); pair_cases<12>(3, 3, 3000); pair_cases<12>(4, 3, 3000);
    pair_cases<8>(4, 2, 3000); pair_cases<8>(3, 2, 3000); pair_cases<6>(3, 2, 3000);
    // the two zips exactly as te_madd_hot instantiates them, every limb at its bound, both signs of the digit (F, G = U, V or V, U)
    const G E = all(3 * U28 - 1), H = all(2 * U28 - 1), U = all(4 * U28 - 1), V = all(3 * U28 - 1), one = all(U28 - 1);
    { const G a3[3] = {all(5 * U28 - 1), H, one}, b3[3] = {one, one, one}; zip<5, 2, 1>(a3, b3, true, "first level"); }
    { const G a4[4] = {E, V, E, U}, b4[4] = {U, H, H, V}; zip<12, 8, 6, 12>(a4, b4, false, "second level, neg = false"); }
    { const G a4[4] = {E, U, E, V}, b4[4] = {V, H, H, U}; zip<12, 8, 6, 12>(a4, b4, false, "second level, neg = true"); }
    for (int i = 0; i < 500; i++) {
        const G e = random_below(3), h = random_below(2), u = random_below(4), v = random_below(3);
        const G a4[4] = {e, v, e, u}, b4[4] = {u, h, h, v};
        zip<12, 8, 6, 12>(a4, b4, false, "second level, random");
        const G a3[3] = {random_below(5), random_below(2), random_below(1)}, b3[3] = {random_below(1), random_below(1), random_below(1)};
        zip<5, 2, 1>(a3, b3, false, "first level, random");
    }
    if (!fallback_needed || !fallback_columns_seen || !zero_columns_seen) { printf("the fallback columns or the t = 0 columns were never exercised\n"); bad++; }
    printf("fq377x28 lower seed: %d products, %d signed columns (%d of them t = 0), %d fallback columns, %d products that need them, %d bad\n",
           products, signed_columns_seen, zero_columns_seen, fallback_columns_seen, fallback_needed, bad);
    return bad ? 1 : 0;
}
