// csrc/fq_sqrt.cuh -- square roots in the BLS12-377 base field and G1 point decompression, ONE implementation for the host compiler (marlin_codec.cpp: Reader::g1,
// the batch verifier's host back end) and for gfx950 (kernels_verify.hip: k_g1_decompress_check, k_fq_sqrt).
//
// Tonelli-Shanks with q - 1 = 2^46 t: from w = a^((t - 1) / 2) alone, x = a w = a^((t + 1) / 2) and b = x w = a^t; b has order 2^i, and i = 46 exactly when a is a
// non-residue (b^(2^45) = a^((q - 1) / 2) = -1), so the Legendre symbol costs no exponentiation of its own.  The constants are computed once on the host (SqrtConsts)
// and handed to a kernel by value.
#pragma once
#include "ec.cuh"

namespace zk {

struct SqrtConsts {
    uint32_t tm1h_limbs[12];   // (t - 1) / 2
    Fq377 z_t;                 // nonresidue^t: a generator of the 2^46-th roots of unity
    int S;                     // 46
};
inline SqrtConsts make_sqrt_consts() {
    SqrtConsts K;
    uint32_t t[12], half[12];
    for (int i = 0; i < 12; i++) t[i] = Fq377P::mod(i);
    t[0] -= 1;
    auto shr1 = [](uint32_t *v) { for (int i = 0; i < 12; i++) v[i] = (v[i] >> 1) | (i < 11 ? v[i + 1] << 31 : 0); };
    memcpy(half, t, sizeof t); shr1(half);
    K.S = 0;
    while (!(t[0] & 1)) { shr1(t); K.S++; }
    memcpy(K.tm1h_limbs, t, sizeof t);
    shr1(K.tm1h_limbs);        // t odd: (t - 1) / 2 = t >> 1
    Fq377 minus_one = Fq377::one().neg();
    for (uint64_t c = 2;; c++) { Fq377 cand = Fq377::from_u64(c); if (cand.pow(half, 12) == minus_one) { K.z_t = cand.pow(t, 12); break; } }
    return K;
}
// C++11 magic static: initialised exactly once, also when the first callers race (verifier-only processes, several threads)
inline const SqrtConsts &sqrt_consts() { static const SqrtConsts K = make_sqrt_consts(); return K; }

// out = a square root of a (which of the two is fixed by the algorithm, the same on host and device); false when a is a non-residue.  sqrt(0) = 0
ZK_HD bool fq_sqrt(const SqrtConsts &K, const Fq377 &a, Fq377 &out) {
    if (a.is_zero()) { out = a; return true; }
    const Fq377 one = Fq377::one();
    Fq377 w = a.pow(K.tm1h_limbs, 12);
    Fq377 x = a * w, b = x * w, c = K.z_t;
    int m = K.S;
    while (!(b == one)) {
        int i = 0;
        Fq377 bb = b;
        while (!(bb == one)) { bb = bb.sqr(); i++; }
        if (i >= m) return false;                    // first round only: the order of b is 2^46, a is a non-residue
        Fq377 g = c;
        for (int k = 0; k < m - i - 1; k++) g = g.sqr();
        x = x * g; c = g.sqr(); b = b * c; m = i;
    }
    out = x;
    return true;
}

// is the canonical integer of y greater than that of -y?  (ark-serialize's sign flag of a compressed point)
ZK_HD bool fq_is_greater_half(const Fq377 &y) {
    uint32_t yr[12], nyr[12];
    y.to_raw(yr); y.neg().to_raw(nyr);
    for (int i = 11; i >= 0; i--) if (yr[i] != nyr[i]) return yr[i] > nyr[i];
    return false;
}

// what a compressed G1 point turns out to be.  G1_MALFORMED is decided from the 48 bytes alone (both flags set, x >= q, an infinity flag over a non-zero x)
enum : uint8_t { G1_OK = 0, G1_INFINITY = 1, G1_NOT_ON_CURVE = 2, G1_NOT_IN_SUBGROUP = 3, G1_MALFORMED = 4 };

// x: canonical limbs (< q), y_gt: the sign flag.  G1_OK: out = the affine point, on the curve and in the prime-order subgroup ([r]P = O, as ark-ec 0.3's
// GroupAffine::deserialize checks: the cofactor is (x - 1)^2 / 3, and a small-order component would survive the pairing check).  The ladder's scalar is r itself, the
// same bits in every lane.
ZK_HD uint8_t g1_decompress_check(const SqrtConsts &K, const uint32_t x_raw[12], bool y_gt, Affine<Fq377> &out) {
    out = Affine<Fq377>::inf();
    Affine<Fq377> a;
    a.x = Fq377::from_raw(x_raw);
    Fq377 y;
    if (!fq_sqrt(K, a.x.sqr() * a.x + Bls377::b(), y)) return G1_NOT_ON_CURVE;
    a.y = (fq_is_greater_half(y) == y_gt) ? y : y.neg();
    uint32_t r[8];
    for (int i = 0; i < 8; i++) r[i] = Fr377P::mod(i);
    if (!XYZZ<Fq377>::from_affine(a).mul_raw(r, 8).is_inf()) return G1_NOT_IN_SUBGROUP;
    out = a;
    return G1_OK;
}

}  // namespace zk
