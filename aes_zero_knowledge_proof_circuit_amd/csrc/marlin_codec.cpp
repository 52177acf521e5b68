// csrc/marlin_codec.cpp -- the host-only half of marlin.hpp: ark-serialize (de)coding of proofs and verifying keys, the replay of KZG10::setup's test_rng draws, and the
// Marlin verifier (src/lib.rs:116-136 -> simpleworks verify_proof -> ark-marlin verify).  Takes UNTRUSTED bytes (proofs, verifying keys): built a second time with
// -fsanitize=address,undefined,fuzzer and driven by tests/fuzz_host.cpp (tests/test_fuzz_host.py); no HIP header is included here.
#include "marlin_host.hpp"
#include <chrono>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <memory>
#include <stdexcept>
#include "transcript.hpp"
#include "fq_sqrt.cuh"
#include "verify_batch.hpp"

namespace zk {
namespace {
using namespace hostx;

// Fq square root for point decompression: fq_sqrt.cuh, shared with the device
bool fq_sqrt(const Fq377 &a, Fq377 &out) { return zk::fq_sqrt(sqrt_consts(), a, out); }

struct Reader {
    const uint8_t *p; size_t n, off = 0;
    void need(size_t k) { if (off + k > n) throw std::runtime_error("deserialize_proof: truncated input"); }
    uint8_t u8() { need(1); return p[off++]; }
    uint64_t u64() { need(8); uint64_t v = 0; for (int i = 0; i < 8; i++) v |= (uint64_t)p[off + i] << (8 * i); off += 8; return v; }
    Fr fr() {
        need(32);
        uint32_t raw[8];
        for (int i = 0; i < 8; i++) raw[i] = (uint32_t)p[off + 4 * i] | (uint32_t)p[off + 4 * i + 1] << 8 | (uint32_t)p[off + 4 * i + 2] << 16 | (uint32_t)p[off + 4 * i + 3] << 24;
        off += 32;
        if (Fr::geq_mod(raw)) throw std::runtime_error("deserialize_proof: non-canonical field element");
        return Fr::from_raw(raw);
    }
    G1A g1() {
        need(48);
        uint8_t buf[48];
        memcpy(buf, p + off, 48); off += 48;
        bool inf = buf[47] & (1 << 6), y_gt = buf[47] & (1 << 7);
        if (inf && y_gt) throw std::runtime_error("deserialize_proof: invalid point flags (infinity and sign both set)");   // ark-serialize SWFlags::from_u8 -> None
        buf[47] &= 0x3f;
        uint32_t raw[12];
        for (int i = 0; i < 12; i++) raw[i] = (uint32_t)buf[4 * i] | (uint32_t)buf[4 * i + 1] << 8 | (uint32_t)buf[4 * i + 2] << 16 | (uint32_t)buf[4 * i + 3] << 24;
        if (Fq377::geq_mod(raw)) throw std::runtime_error("deserialize_proof: non-canonical x coordinate");
        if (inf) {
            for (int i = 0; i < 12; i++) if (raw[i]) throw std::runtime_error("deserialize_proof: point at infinity with a non-zero x coordinate");   // one encoding per point
            return G1A::inf();
        }
        G1A a;
        // ark-ec 0.3 GroupAffine::deserialize: is_in_correct_subgroup_assuming_on_curve, i.e. [r]P == O (the curve has cofactor (x-1)^2/3: a
        // small-order component would survive the pairing check and make proofs malleable)
        switch (g1_decompress_check(sqrt_consts(), raw, y_gt, a)) {
            case G1_NOT_ON_CURVE: throw std::runtime_error("deserialize_proof: x is not on the curve");
            case G1_NOT_IN_SUBGROUP: throw std::runtime_error("deserialize_proof: point is not in the prime-order subgroup");
            default: break;
        }
        return a;
    }
};


// Fq2 = Fq[u]/(u^2 + 5): lexicographic order of ark-ff's QuadExtField (c1 first, then c0) for the compressed-point sign flag
bool fq2_gt(const pairing::Fq2 &a, const pairing::Fq2 &b) {
    uint32_t x[12], y[12];
    a.c1.to_raw(x); b.c1.to_raw(y);
    for (int i = 11; i >= 0; i--) if (x[i] != y[i]) return x[i] > y[i];
    a.c0.to_raw(x); b.c0.to_raw(y);
    for (int i = 11; i >= 0; i--) if (x[i] != y[i]) return x[i] > y[i];
    return false;
}
// square root in Fq2 through the norm: a = a0 + a1 u, alpha = sqrt(a0^2 + 5 a1^2), delta = (a0 +- alpha)/2, c0 = sqrt(delta), c1 = a1/(2 c0)
bool fq2_sqrt(const pairing::Fq2 &a, pairing::Fq2 &out) {
    using pairing::Fq2;
    if (a.is_zero()) { out = a; return true; }
    Fq377 inv2 = Fq377::from_u64(2).inverse();
    if (a.c1.is_zero()) {
        Fq377 r;
        if (fq_sqrt(a.c0, r)) { out = Fq2{r, Fq377::zero()}; return true; }
        if (!fq_sqrt((a.c0 * Fq377::from_u64(5).inverse()).neg(), r)) return false;
        out = Fq2{Fq377::zero(), r};
        return true;
    }
    Fq377 alpha;
    if (!fq_sqrt(a.c0.sqr() + pairing::times5(a.c1.sqr()), alpha)) return false;
    Fq377 delta = (a.c0 + alpha) * inv2, c0;
    if (!fq_sqrt(delta, c0)) { delta = (a.c0 - alpha) * inv2; if (!fq_sqrt(delta, c0)) return false; }
    out = Fq2{c0, a.c1 * (c0.dbl()).inverse()};
    return out.sqr() == a;
}
void put_g2_compressed(Bytes &o, const pairing::G2Affine &p) {
    uint8_t buf[96] = {0};
    if (p.inf) { buf[95] |= 1 << 6; o.put(buf, 96); return; }
    uint32_t x0[12], x1[12];
    p.x.c0.to_raw(x0); p.x.c1.to_raw(x1);
    for (int i = 0; i < 48; i++) { buf[i] = (uint8_t)(x0[i / 4] >> (8 * (i % 4))); buf[48 + i] = (uint8_t)(x1[i / 4] >> (8 * (i % 4))); }
    if (fq2_gt(p.y, p.y.neg())) buf[95] |= 1 << 7;
    o.put(buf, 96);
}
void put_g2_uncompressed(Bytes &o, const pairing::G2Affine &p) {       // x (c0, c1), y (c0, c1 with the flags byte): 192 bytes
    const size_t at = o.b.size();
    if (p.inf) { for (int i = 0; i < 2; i++) o.field(Fq377::zero()); o.field(Fq377::one()); o.field(Fq377::zero()); o.b[at + 191] |= 1 << 6; return; }
    o.field(p.x.c0); o.field(p.x.c1); o.field(p.y.c0); o.field(p.y.c1);
}
pairing::G2Affine get_g2_compressed(Reader &r) {
    r.need(96);
    uint8_t buf[96];
    memcpy(buf, r.p + r.off, 96); r.off += 96;
    bool inf = buf[95] & (1 << 6), y_gt = buf[95] & (1 << 7);
    if (inf && y_gt) throw std::runtime_error("deserialize: invalid G2 point flags (infinity and sign both set)");
    buf[95] &= 0x3f;
    uint32_t raw[2][12];
    for (int h = 0; h < 2; h++) {
        for (int i = 0; i < 12; i++) { const uint8_t *q = buf + 48 * h + 4 * i; raw[h][i] = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24; }
        if (Fq377::geq_mod(raw[h])) throw std::runtime_error("deserialize: non-canonical G2 x coordinate");
    }
    if (inf) {
        for (int h = 0; h < 2; h++) for (int i = 0; i < 12; i++) if (raw[h][i]) throw std::runtime_error("deserialize: G2 point at infinity with a non-zero x coordinate");
        return pairing::G2Affine::infinity();
    }
    pairing::G2Affine a;
    a.inf = false;
    a.x = pairing::Fq2{Fq377::from_raw(raw[0]), Fq377::from_raw(raw[1])};
    pairing::Fq2 y;
    if (!fq2_sqrt(a.x.sqr() * a.x + pairing::g2_b(), y)) throw std::runtime_error("deserialize: G2 x is not on the twist");
    a.y = (fq2_gt(y, y.neg()) == y_gt) ? y : y.neg();
    if (!pairing::g2_mul_raw(a, FR377_P, 8).inf) throw std::runtime_error("deserialize: G2 point is not in the prime-order subgroup");
    return a;
}


// canonical-integer comparison a < b (ark-ff's Ord on Fp)
bool fq_lt(const Fq377 &a, const Fq377 &b) {
    uint32_t x[12], y[12];
    a.to_raw(x); b.to_raw(y);
    for (int i = 11; i >= 0; i--) if (x[i] != y[i]) return x[i] < y[i];
    return false;
}
// ark-ec 0.3.0 `impl Distribution<GroupProjective<P>> for Standard` [RECALL]: loop { x = BaseField::rand; greatest = rng.gen::<bool>();
// get_point_from_x(x, greatest) } then scale_by_cofactor.  gen::<bool>() = top bit of one next_u32; y = (y < -y) ^ greatest ? y : -y.
G1A sample_g1(ChaChaRng &rng) {
    for (;;) {
        Fq377 x = rng.rand_field<Fq377>();
        bool greatest = (rng.next_u32() >> 31) != 0;
        Fq377 y;
        if (!fq_sqrt(x.sqr() * x + Bls377::b(), y)) continue;
        Fq377 ny = y.neg();
        G1A p; p.x = x; p.y = (fq_lt(y, ny) != greatest) ? y : ny;
        return XYZZ<Fq377>::from_affine(p).mul_raw(G1_377_COFACTOR, G1_377_COFACTOR_LIMBS).to_affine();
    }
}
pairing::G2Affine sample_g2(ChaChaRng &rng) {
    using pairing::Fq2;
    for (;;) {
        Fq2 x;
        x.c0 = rng.rand_field<Fq377>(); x.c1 = rng.rand_field<Fq377>();          // QuadExtField::rand: c0 then c1
        bool greatest = (rng.next_u32() >> 31) != 0;
        Fq2 y;
        if (!fq2_sqrt(x.sqr() * x + pairing::g2_b(), y)) continue;
        Fq2 ny = y.neg();
        pairing::G2Affine p; p.inf = false; p.x = x; p.y = (fq2_gt(ny, y) != greatest) ? y : ny;    // (y < -y) ^ greatest
        return pairing::g2_mul_raw(p, G2_377_COFACTOR, G2_377_COFACTOR_LIMBS);
    }
}

}  // namespace

// KZG10::setup's draws from ark_std::test_rng(), in upstream's order [RECALL ark-poly-commit 0.3.0]: beta, g, gamma_g, h
void kzg_setup_points(Fr &beta, G1A &g, G1A &gamma_g, pairing::G2Affine &h) {
    ChaChaRng rng(ark_test_rng_seed(), 12);
    beta = rng.rand_field<Fr>();
    g = sample_g1(rng);
    gamma_g = sample_g1(rng);
    h = sample_g2(rng);
}

// ark-serialize 0.3 compressed layout of ark_marlin::IndexVerifierKey<Fr, MarlinKZG10<Bls12_377, _>> [RECALL, SURVEY.md A.5]:
//   index_info   : num_variables, num_constraints, num_non_zero, num_instance_variables            (4 x u64 LE; PhantomData = 0 bytes)
//   index_comms  : u64 len, then per marlin_pc::Commitment: comm (G1 compressed 48 B), shifted_comm Option tag (0 = None)
//   verifier_key : marlin_pc::VerifierKey = kzg10::VerifierKey { g, gamma_g (G1 48 B each), h, beta_h (G2 compressed 96 B each); the
//                  prepared G2 elements are not serialized }, degree_bounds_and_shift_powers Option<Vec<(usize, G1)>> (tag, u64 len,
//                  (u64, 48 B) each), max_degree u64, supported_degree u64
// `uncompressed`: the image serialize_uncompressed writes (G1 96 B, G2 192 B, everything else identical) -- the form deserialize_unchecked reads
std::vector<uint8_t> serialize_vk_ark(const VerifyingKey &vk, bool uncompressed) {
    Bytes o;
    auto g2 = [&](const pairing::G2Affine &p) { if (uncompressed) put_g2_uncompressed(o, p); else put_g2_compressed(o, p); };
    o.u64(vk.num_variables); o.u64(vk.num_constraints); o.u64(vk.num_non_zero); o.u64(vk.num_instance);
    o.u64(6);
    for (int i = 0; i < 6; i++) { o.g1(vk.index_comms[i], uncompressed); o.u8(0); }
    o.g1(vk.g, uncompressed); o.g1(vk.gamma_g, uncompressed);
    g2(vk.h); g2(vk.beta_h);
    o.u8(1); o.u64(2);
    for (int i = 0; i < 2; i++) { o.u64(vk.degree_bounds[i]); o.g1(vk.shift_powers[i], uncompressed); }
    o.u64(vk.max_degree); o.u64(vk.supported_degree);
    return o.b;
}
VerifyingKey deserialize_vk_ark(const uint8_t *bytes, size_t len) {
    Reader r{bytes, len};
    VerifyingKey vk;
    vk.num_variables = r.u64(); vk.num_constraints = r.u64(); vk.num_non_zero = r.u64(); vk.num_instance = r.u64();
    if (r.u64() != 6) throw std::runtime_error("deserialize_vk: expected 6 index commitments");
    for (int i = 0; i < 6; i++) { vk.index_comms[i] = r.g1(); if (r.u8() != 0) throw std::runtime_error("deserialize_vk: index commitments carry no degree bound"); }
    vk.g = r.g1(); vk.gamma_g = r.g1();
    vk.h = get_g2_compressed(r); vk.beta_h = get_g2_compressed(r);
    if (r.u8() != 1 || r.u64() != 2) throw std::runtime_error("deserialize_vk: expected two enforced degree bounds");
    for (int i = 0; i < 2; i++) { vk.degree_bounds[i] = (size_t)r.u64(); vk.shift_powers[i] = r.g1(); }
    vk.max_degree = (size_t)r.u64(); vk.supported_degree = (size_t)r.u64();
    if (r.off != len) throw std::runtime_error("deserialize_vk: trailing bytes");
    if (vk.num_instance == 0 || vk.num_variables < vk.num_instance) throw std::runtime_error("deserialize_vk: inconsistent index info");
    // sizes a radix-2 domain of Fr (two-adicity 47) can hold; anything larger is not a key this library (or ark-marlin) could have produced, and the verifier's
    // domain arithmetic (next_pow2, roots of unity) is only defined below it
    const uint64_t LIM = (uint64_t)1 << 46;
    if (vk.num_variables > LIM || vk.num_constraints > LIM || vk.num_non_zero > LIM || vk.num_constraints == 0 || vk.num_non_zero == 0) throw std::runtime_error("deserialize_vk: index sizes out of range");
    if (vk.max_degree > 3 * LIM || vk.supported_degree > vk.max_degree || vk.degree_bounds[0] > vk.degree_bounds[1] || vk.degree_bounds[1] > vk.max_degree)
        throw std::runtime_error("deserialize_vk: inconsistent degree bounds");
    vk.num_public_inputs = (size_t)vk.num_instance - 1;   // the padded count; the verifier zero-pads shorter inputs the same way
    return vk;
}

std::vector<uint8_t> serialize_proof(const Proof &p) {
    Bytes o;
    static const int round_len[3] = {4, 3, 2};
    o.u64(3);
    int ci = 0;
    for (int r = 0; r < 3; r++) {
        o.u64(round_len[r]);
        for (int i = 0; i < round_len[r]; i++, ci++) {
            o.g1_compressed(p.comms[ci].comm);
            o.u8(p.comms[ci].has_shifted ? 1 : 0);
            if (p.comms[ci].has_shifted) o.g1_compressed(p.comms[ci].shifted);
        }
    }
    o.u64(4);
    for (int i = 0; i < 4; i++) o.field(p.evals[i]);
    o.u64(3);
    for (int i = 0; i < 3; i++) o.u8(0);                 // prover_messages: EmptyMessage -> Option::None
    o.u64(2);
    o.g1_compressed(p.w_beta); o.u8(1); o.field(p.random_v_beta);
    o.g1_compressed(p.w_gamma); o.u8(0);
    o.u8(0);                                             // pc_proof.evals: None
    return o.b;
}
Proof deserialize_proof(const uint8_t *bytes, size_t len) {
    Reader r{bytes, len};
    Proof p;
    static const uint64_t round_len[3] = {4, 3, 2};
    if (r.u64() != 3) throw std::runtime_error("deserialize_proof: expected 3 commitment rounds");
    int ci = 0;
    for (int rd = 0; rd < 3; rd++) {
        if (r.u64() != round_len[rd]) throw std::runtime_error("deserialize_proof: unexpected number of commitments");
        for (uint64_t i = 0; i < round_len[rd]; i++, ci++) {
            p.comms[ci].comm = r.g1();
            uint8_t tag = r.u8();
            if (tag > 1) throw std::runtime_error("deserialize_proof: bad Option tag");
            p.comms[ci].has_shifted = tag;
            if (tag) p.comms[ci].shifted = r.g1();
        }
    }
    if (r.u64() != 4) throw std::runtime_error("deserialize_proof: expected 4 evaluations");
    for (int i = 0; i < 4; i++) p.evals[i] = r.fr();
    if (r.u64() != 3) throw std::runtime_error("deserialize_proof: expected 3 prover messages");
    for (int i = 0; i < 3; i++) if (r.u8() != 0) throw std::runtime_error("deserialize_proof: non-empty prover message");
    if (r.u64() != 2) throw std::runtime_error("deserialize_proof: expected 2 opening proofs");
    p.w_beta = r.g1();
    if (r.u8() != 1) throw std::runtime_error("deserialize_proof: opening 0 must carry random_v");
    p.random_v_beta = r.fr();
    p.w_gamma = r.g1();
    if (r.u8() != 0) throw std::runtime_error("deserialize_proof: opening 1 must not carry random_v");
    if (r.u8() != 0) throw std::runtime_error("deserialize_proof: unexpected pc_proof.evals");
    if (r.off != len) throw std::runtime_error("deserialize_proof: trailing bytes");
    return p;
}

std::vector<Fr> ciphertext_to_public_input(const uint8_t *ct, size_t len) {
    std::vector<Fr> v;
    v.reserve(len * 8);
    for (size_t i = 0; i < len; i++) for (int b = 0; b < 8; b++) v.push_back(((ct[i] >> b) & 1) ? Fr::one() : Fr::zero());
    return v;
}

// =====================================================================================================================
// verifier (host only)
bool verify(const VerifyingKey &vk, const std::vector<Fr> &public_input_in, const Proof &proof) {
    using X = XYZZ<Fq377>;
    // pad the public input to |X| - 1 (ark-marlin verify)
    size_t m = next_pow2(public_input_in.size() + 1);
    std::vector<Fr> pub(public_input_in);
    pub.resize(std::max(public_input_in.size(), m - 1), Fr::zero());
    if (m != vk.num_instance) return false;               // InvalidPublicInputLength / instance does not match the index
    size_t n = next_pow2(vk.num_constraints), k = next_pow2(vk.num_non_zero);
    FiatShamirRng fs;
    {
        Bytes o;
        o.put("MARLIN-2019", 11);
        o.u64(vk.num_variables); o.u64(vk.num_constraints); o.u64(vk.num_non_zero);
        for (int i = 0; i < 6; i++) { Commitment ic; ic.comm = vk.index_comms[i]; o.commitment_tobytes(ic); }
        for (auto &v : pub) o.field(v);
        fs.initialize(o.b);
    }
    auto absorb_comms = [&](int from, int cnt) { Bytes o; for (int i = 0; i < cnt; i++) o.commitment_tobytes(proof.comms[from + i]); fs.absorb(o.b); };
    auto sample_outside_h = [&]() { Fr t; do { t = fs.rng().rand_field<Fr>(); } while (eval_vanishing(n, t).is_zero()); return t; };
    absorb_comms(0, 4);
    Fr alpha = sample_outside_h();
    Fr eta_a = fs.rng().rand_field<Fr>(), eta_b = fs.rng().rand_field<Fr>(), eta_c = fs.rng().rand_field<Fr>();
    absorb_comms(4, 3);
    Fr beta = sample_outside_h();
    absorb_comms(7, 2);
    Fr gamma = fs.rng().rand_field<Fr>();
    { Bytes o; for (auto &v : proof.evals) o.field(v); fs.absorb(o.b); }
    Fr ch;
    { uint64_t lo = fs.rng().next_u64(), hi = fs.rng().next_u64(); uint32_t raw[8] = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32), 0, 0, 0, 0}; ch = Fr::from_raw(raw); }
    // degree-bound shape checks (commitments g_1, g_2 carry shifted parts, the others must not)
    for (int i = 0; i < 9; i++) if (proof.comms[i].has_shifted != (i == 5 || i == 7)) return false;
    const Fr g1_b = proof.evals[0], g2_g = proof.evals[1], t_b = proof.evals[2], zb_b = proof.evals[3];
    // ---- construct_linear_combinations
    Fr vh_alpha = eval_vanishing(n, alpha), vh_beta = eval_vanishing(n, beta), vx_beta = eval_vanishing(m, beta), vk_gamma = eval_vanishing(k, gamma);
    Fr r_alpha_at_beta = (vh_alpha - vh_beta) * (alpha - beta).inverse();
    // x(beta) = sum_i L_i(beta) x_i over the X domain, x = [1, public inputs...]
    Fr x_at_beta = Fr::zero();
    {
        int lg_m = log2_exact(m);
        Fr gx = domain_gen(lg_m), m_inv = Fr::from_u64(m).inverse();
        if (vx_beta.is_zero()) {                                   // beta in X: the Lagrange basis is an indicator
            Fr e = Fr::one();
            for (size_t i = 0; i < m; i++) { if (e == beta) x_at_beta = i == 0 ? Fr::one() : pub[i - 1]; e = e * gx; }
        } else {
            // L_i(beta) = v_X(beta) * g^i / (m * (beta - g^i))
            std::vector<Fr> den(m);
            Fr e = Fr::one();
            for (size_t i = 0; i < m; i++) { den[i] = beta - e; e = e * gx; }
            // batch inversion
            std::vector<Fr> pre(m);
            Fr accp = Fr::one();
            for (size_t i = 0; i < m; i++) { pre[i] = accp; accp = accp * den[i]; }
            Fr inv = accp.inverse();
            for (size_t i = m; i-- > 0;) { Fr d = den[i]; den[i] = inv * pre[i]; inv = inv * d; }
            e = Fr::one();
            Fr common = vx_beta * m_inv;
            for (size_t i = 0; i < m; i++) {
                const Fr xi = i == 0 ? Fr::one() : pub[i - 1];
                if (!xi.is_zero()) x_at_beta = x_at_beta + common * e * den[i] * xi;
                e = e * gx;
            }
        }
    }
    Fr bmul = gamma * g2_g + t_b * Fr::from_u64(k).inverse();
    Fr vv = vh_alpha * vh_beta;
    // commitments by label
    const G1A &C_w = proof.comms[0].comm, &C_za = proof.comms[1].comm, &C_zb = proof.comms[2].comm, &C_mask = proof.comms[3].comm;
    const G1A &C_t = proof.comms[4].comm, &C_g1 = proof.comms[5].comm, &C_h1 = proof.comms[6].comm, &C_g2 = proof.comms[7].comm, &C_h2 = proof.comms[8].comm;
    const G1A *IX = vk.index_comms;   // row col a_val b_val c_val row_col
    auto add_scaled = [](X &acc, const G1A &c, const Fr &s) { if (s == Fr::one()) acc.madd(c); else acc.add(mul_fr(X::from_affine(c), s)); };
    // outer_sumcheck: commitment and expected evaluation (constants moved to the evaluation side, check_combinations)
    X outer = X::inf();
    add_scaled(outer, C_mask, Fr::one());
    add_scaled(outer, C_za, r_alpha_at_beta * (eta_a + eta_c * zb_b));
    add_scaled(outer, C_w, (t_b * vx_beta).neg());
    add_scaled(outer, C_h1, vh_beta.neg());
    Fr outer_eval = Fr::zero() - (r_alpha_at_beta * eta_b * zb_b) - ((t_b * x_at_beta).neg()) - ((beta * g1_b).neg());
    X inner = X::inf();
    add_scaled(inner, IX[2], eta_a * vv); add_scaled(inner, IX[3], eta_b * vv); add_scaled(inner, IX[4], eta_c * vv);
    add_scaled(inner, IX[0], alpha * bmul); add_scaled(inner, IX[1], beta * bmul); add_scaled(inner, IX[5], bmul.neg());
    add_scaled(inner, C_h2, vk_gamma.neg());
    Fr inner_eval = Fr::zero() - ((alpha * beta * bmul).neg());
    // ---- combine_and_normalize per query point (labels in BTreeSet order)
    Fr chp[5]; chp[0] = Fr::one(); for (int i = 1; i < 5; i++) chp[i] = chp[i - 1] * ch;
    auto shift_power = [&](size_t bound) -> const G1A & { return bound == vk.degree_bounds[0] ? vk.shift_powers[0] : vk.shift_powers[1]; };
    // beta: g_1 (ch^0, shifted ch^1), outer_sumcheck (ch^2), t (ch^3), z_b (ch^4)
    X comb_b = X::inf(); Fr val_b = Fr::zero();
    add_scaled(comb_b, C_g1, chp[0]); val_b = val_b + g1_b * chp[0];
    { X adj = X::from_affine(proof.comms[5].shifted); adj.add(mul_fr(X::from_affine(shift_power(n - 2)), g1_b).neg()); comb_b.add(mul_fr(adj, chp[1])); }
    comb_b.add(mul_fr(outer, chp[2])); val_b = val_b + outer_eval * chp[2];
    add_scaled(comb_b, C_t, chp[3]); val_b = val_b + t_b * chp[3];
    add_scaled(comb_b, C_zb, chp[4]); val_b = val_b + zb_b * chp[4];
    // gamma: g_2 (ch^0, shifted ch^1), inner_sumcheck (ch^2)
    X comb_g = X::inf(); Fr val_g = Fr::zero();
    add_scaled(comb_g, C_g2, chp[0]); val_g = val_g + g2_g * chp[0];
    { X adj = X::from_affine(proof.comms[7].shifted); adj.add(mul_fr(X::from_affine(shift_power(k - 2)), g2_g).neg()); comb_g.add(mul_fr(adj, chp[1])); }
    comb_g.add(mul_fr(inner, chp[2])); val_g = val_g + inner_eval * chp[2];
    // ---- KZG10::batch_check with 128-bit randomizers from generate_rand()
    ChaChaRng vrng(ark_test_rng_seed(), 12);
    X total_c = X::inf(), total_w = X::inf();
    Fr g_mult = Fr::zero(), gg_mult = Fr::zero(), randomizer = Fr::one();
    struct Item { X c; Fr z, v; const G1A *w; bool has_rv; Fr rv; } items[2] = {{comb_b, beta, val_b, &proof.w_beta, true, proof.random_v_beta}, {comb_g, gamma, val_g, &proof.w_gamma, false, Fr::zero()}};
    for (auto &it : items) {
        X tmp = mul_fr(X::from_affine(*it.w), it.z);
        tmp.add(it.c);
        g_mult = g_mult + randomizer * it.v;
        if (it.has_rv) gg_mult = gg_mult + randomizer * it.rv;
        total_c.add(mul_fr(tmp, randomizer));
        total_w.add(mul_fr(X::from_affine(*it.w), randomizer));
        uint64_t lo = vrng.next_u64(), hi = vrng.next_u64();
        uint32_t raw[8] = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32), 0, 0, 0, 0};
        randomizer = Fr::from_raw(raw);
    }
    total_c.add(mul_fr(X::from_affine(vk.g), g_mult).neg());
    total_c.add(mul_fr(X::from_affine(vk.gamma_g), gg_mult).neg());
    G1A Ps[2] = {total_w.neg().to_affine(), total_c.to_affine()};
    pairing::G2Affine Qs[2] = {vk.beta_h, vk.h};
    return pairing::pairing_product_is_one(Ps, Qs, 2);
}

// =====================================================================================================================
// batch verifier (verify_batch.hpp): what verify() above does per proof up to its two Items, kept as scalars over base points; a random linear
// combination of all 2n opening equations; two MSMs and one product of two pairings per (sub-)batch
bool g1_parse_compressed(const uint8_t bytes[48], G1Compressed &out, bool *inf_out) {
    uint8_t buf[48];
    memcpy(buf, bytes, 48);
    const bool inf = buf[47] & (1 << 6), y_gt = buf[47] & (1 << 7);
    if (inf && y_gt) return false;
    buf[47] &= 0x3f;
    for (int i = 0; i < 12; i++) out.x[i] = (uint32_t)buf[4 * i] | (uint32_t)buf[4 * i + 1] << 8 | (uint32_t)buf[4 * i + 2] << 16 | (uint32_t)buf[4 * i + 3] << 24;
    out.y_gt = y_gt ? 1 : 0;
    if (Fq377::geq_mod(out.x)) return false;
    if (inf) for (int i = 0; i < 12; i++) if (out.x[i]) return false;
    *inf_out = inf;
    return true;
}

namespace {
using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

// a proof's bytes with its 13 points still compressed; the layout and every check of deserialize_proof, the has_shifted shapes of verify()
struct RawProof {
    G1Compressed pts[VB_OWN];
    bool inf[VB_OWN];
    Fr evals[4], random_v_beta;
};
bool parse_raw_proof(const uint8_t *bytes, size_t len, RawProof &p) {
    size_t off = 0;
    auto u8 = [&](uint8_t &v) { if (off + 1 > len) return false; v = bytes[off++]; return true; };
    auto u64 = [&](uint64_t &v) { if (len - off < 8 || off > len) return false; v = 0; for (int i = 0; i < 8; i++) v |= (uint64_t)bytes[off + i] << (8 * i); off += 8; return true; };
    auto expect64 = [&](uint64_t want) { uint64_t v; return u64(v) && v == want; };
    auto expect8 = [&](uint8_t want) { uint8_t v; return u8(v) && v == want; };
    auto fr = [&](Fr &v) {
        if (len - off < 32) return false;
        uint32_t raw[8];
        for (int i = 0; i < 8; i++) raw[i] = (uint32_t)bytes[off + 4 * i] | (uint32_t)bytes[off + 4 * i + 1] << 8 | (uint32_t)bytes[off + 4 * i + 2] << 16 | (uint32_t)bytes[off + 4 * i + 3] << 24;
        off += 32;
        if (Fr::geq_mod(raw)) return false;
        v = Fr::from_raw(raw);
        return true;
    };
    auto g1 = [&](int slot) {
        if (len - off < 48) return false;
        bool ok = g1_parse_compressed(bytes + off, p.pts[slot], &p.inf[slot]);
        off += 48;
        return ok;
    };
    static const uint64_t round_len[3] = {4, 3, 2};
    if (!expect64(3)) return false;
    int ci = 0, slot = 0;
    for (int rd = 0; rd < 3; rd++) {
        if (!expect64(round_len[rd])) return false;
        for (uint64_t i = 0; i < round_len[rd]; i++, ci++) {
            if (!g1(slot++)) return false;
            uint8_t tag;
            if (!u8(tag) || tag != ((ci == 5 || ci == 7) ? 1 : 0)) return false;      // a bad Option tag, or a degree-bound shape verify() rejects
            if (tag && !g1(slot++)) return false;
        }
    }
    if (!expect64(4)) return false;
    for (int i = 0; i < 4; i++) if (!fr(p.evals[i])) return false;
    if (!expect64(3)) return false;
    for (int i = 0; i < 3; i++) if (!expect8(0)) return false;
    if (!expect64(2)) return false;
    if (!g1(11) || !expect8(1) || !fr(p.random_v_beta)) return false;
    if (!g1(12) || !expect8(0) || !expect8(0)) return false;
    return off == len;
}

// the slots of a proof's own bases
enum { S_W = 0, S_ZA, S_ZB, S_MASK, S_T, S_G1, S_G1S, S_H1, S_G2, S_G2S, S_H2, S_WB, S_WG };
// ... and of the key's
enum { K_IX = 0, K_SP = 6, K_G = 8, K_GG = 9 };

struct Challenges { Fr alpha, eta_a, eta_b, eta_c, beta, gamma, ch; };
struct Rows { Fr own[VB_OWN], shared[VB_SHARED], w[2]; };

// the per-key part of the transcript's first message
Bytes transcript_prefix(const VerifyingKey &vk) {
    Bytes o;
    o.put("MARLIN-2019", 11);
    o.u64(vk.num_variables); o.u64(vk.num_constraints); o.u64(vk.num_non_zero);
    for (int i = 0; i < 6; i++) { Commitment ic; ic.comm = vk.index_comms[i]; o.commitment_tobytes(ic); }
    return o;
}
Challenges run_transcript(const Bytes &prefix, size_t n, size_t m, const uint8_t *bits, size_t n_bits, const G1A *own, const Fr *evals) {
    Challenges c;
    FiatShamirRng fs;
    {
        Bytes o = prefix;
        Bytes enc[2];
        enc[0].field(Fr::zero()); enc[1].field(Fr::one());
        o.b.reserve(o.b.size() + 32 * m);
        for (size_t i = 0; i + 1 < m; i++) { const Bytes &e = enc[i < n_bits && bits[i] ? 1 : 0]; o.b.insert(o.b.end(), e.b.begin(), e.b.end()); }
        fs.initialize(o.b);
    }
    auto comm = [&](int slot, int shifted_slot) { Commitment k; k.comm = own[slot]; if (shifted_slot >= 0) { k.has_shifted = true; k.shifted = own[shifted_slot]; } return k; };
    auto absorb = [&](std::initializer_list<Commitment> cs) { Bytes o; for (auto &k : cs) o.commitment_tobytes(k); fs.absorb(o.b); };
    auto sample_outside_h = [&]() { Fr t; do { t = fs.rng().rand_field<Fr>(); } while (eval_vanishing(n, t).is_zero()); return t; };
    absorb({comm(S_W, -1), comm(S_ZA, -1), comm(S_ZB, -1), comm(S_MASK, -1)});
    c.alpha = sample_outside_h();
    c.eta_a = fs.rng().rand_field<Fr>(); c.eta_b = fs.rng().rand_field<Fr>(); c.eta_c = fs.rng().rand_field<Fr>();
    absorb({comm(S_T, -1), comm(S_G1, S_G1S), comm(S_H1, -1)});
    c.beta = sample_outside_h();
    absorb({comm(S_G2, S_G2S), comm(S_H2, -1)});
    c.gamma = fs.rng().rand_field<Fr>();
    { Bytes o; for (int i = 0; i < 4; i++) o.field(evals[i]); fs.absorb(o.b); }
    { uint64_t lo = fs.rng().next_u64(), hi = fs.rng().next_u64(); uint32_t raw[8] = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32), 0, 0, 0, 0}; c.ch = Fr::from_raw(raw); }
    return c;
}
// verify()'s construct_linear_combinations and combine_and_normalize as scalars: equation beta weighted by rb, equation gamma by rg
Rows scalar_rows(const VerifyingKey &vk, size_t n, size_t m, size_t k, const Challenges &c, const Fr &x_at_beta, const Fr *evals, const Fr &random_v_beta, const Fr &rb, const Fr &rg) {
    Rows R;
    for (auto &v : R.own) v = Fr::zero();
    for (auto &v : R.shared) v = Fr::zero();
    const Fr &alpha = c.alpha, &beta = c.beta, &gamma = c.gamma;
    const Fr g1_b = evals[0], g2_g = evals[1], t_b = evals[2], zb_b = evals[3];
    Fr vh_alpha = eval_vanishing(n, alpha), vh_beta = eval_vanishing(n, beta), vx_beta = eval_vanishing(m, beta), vk_gamma = eval_vanishing(k, gamma);
    Fr r_alpha_at_beta = (vh_alpha - vh_beta) * (alpha - beta).inverse();
    Fr bmul = gamma * g2_g + t_b * Fr::from_u64(k).inverse();
    Fr vv = vh_alpha * vh_beta;
    Fr outer_eval = Fr::zero() - (r_alpha_at_beta * c.eta_b * zb_b) - ((t_b * x_at_beta).neg()) - ((beta * g1_b).neg());
    Fr inner_eval = Fr::zero() - ((alpha * beta * bmul).neg());
    Fr chp[5]; chp[0] = Fr::one(); for (int i = 1; i < 5; i++) chp[i] = chp[i - 1] * c.ch;
    auto sp = [&](size_t bound) { return K_SP + (bound == vk.degree_bounds[0] ? 0 : 1); };
    // beta: g_1 (ch^0, shifted ch^1), outer_sumcheck (ch^2), t (ch^3), z_b (ch^4)
    const Fr ob = rb * chp[2];
    R.own[S_G1] = rb; R.own[S_G1S] = rb * chp[1];
    R.shared[sp(n - 2)] = R.shared[sp(n - 2)] - rb * chp[1] * g1_b;
    R.own[S_MASK] = ob;
    R.own[S_ZA] = ob * r_alpha_at_beta * (c.eta_a + c.eta_c * zb_b);
    R.own[S_W] = ob * (t_b * vx_beta).neg();
    R.own[S_H1] = ob * vh_beta.neg();
    R.own[S_T] = rb * chp[3];
    R.own[S_ZB] = rb * chp[4];
    Fr val_b = g1_b + outer_eval * chp[2] + t_b * chp[3] + zb_b * chp[4];
    // gamma: g_2 (ch^0, shifted ch^1), inner_sumcheck (ch^2)
    const Fr og = rg * chp[2];
    R.own[S_G2] = rg; R.own[S_G2S] = rg * chp[1];
    R.shared[sp(k - 2)] = R.shared[sp(k - 2)] - rg * chp[1] * g2_g;
    R.shared[K_IX + 2] = og * c.eta_a * vv; R.shared[K_IX + 3] = og * c.eta_b * vv; R.shared[K_IX + 4] = og * c.eta_c * vv;
    R.shared[K_IX + 0] = og * alpha * bmul; R.shared[K_IX + 1] = og * beta * bmul; R.shared[K_IX + 5] = og * bmul.neg();
    R.own[S_H2] = og * vk_gamma.neg();
    Fr val_g = g2_g + inner_eval * chp[2];
    // z W + C - v g - rv gamma_g on the h side, -W on the beta_h side
    R.own[S_WB] = rb * beta; R.own[S_WG] = rg * gamma;
    R.shared[K_G] = (rb * val_b + rg * val_g).neg();
    R.shared[K_GG] = (rb * random_v_beta).neg();
    R.w[0] = rb; R.w[1] = rg;
    return R;
}

// x^(beta) as verify() computes it
Fr host_public_input_eval(int lg_m, const Fr &beta, const uint8_t *bits, size_t n_bits) {
    const size_t m = (size_t)1 << lg_m;
    auto xi = [&](size_t i) { return i == 0 || (i - 1 < n_bits && bits[i - 1]); };
    Fr gx = domain_gen(lg_m), vx_beta = eval_vanishing(m, beta), acc = Fr::zero();
    if (vx_beta.is_zero()) {                                   // beta in X: the Lagrange basis is an indicator
        Fr e = Fr::one();
        for (size_t i = 0; i < m; i++) { if (e == beta) acc = xi(i) ? Fr::one() : Fr::zero(); e = e * gx; }
        return acc;
    }
    // L_i(beta) = v_X(beta) * g^i / (m * (beta - g^i)), one inversion for all of them
    std::vector<Fr> den(m), pre(m);
    Fr e = Fr::one(), accp = Fr::one();
    for (size_t i = 0; i < m; i++) { den[i] = beta - e; e = e * gx; pre[i] = accp; accp = accp * den[i]; }
    Fr inv = accp.inverse();
    for (size_t i = m; i-- > 0;) { Fr d = den[i]; den[i] = inv * pre[i]; inv = inv * d; }
    e = Fr::one();
    for (size_t i = 0; i < m; i++) { if (xi(i)) acc = acc + e * den[i]; e = e * gx; }
    return acc * vx_beta * Fr::from_u64(m).inverse();
}

// bucket method on the host's XYZZ code (complete: madd covers P = +-Q and infinity bases); `bits` = the scalars' width
XYZZ<Fq377> host_msm(const G1A *bases, const Fr *scalars, size_t n, int bits) {
    using X = XYZZ<Fq377>;
    std::vector<uint32_t> raw(8 * n);
    for (size_t i = 0; i < n; i++) scalars[i].to_raw(&raw[8 * i]);
    const int c = n < 8 ? 2 : n < 64 ? 4 : n < 1024 ? 6 : n < 16384 ? 9 : 12, nwin = (bits + c - 1) / c;
    std::vector<X> buckets(((size_t)1 << c) - 1);
    X total = X::inf();
    for (int w = nwin - 1; w >= 0; w--) {
        for (int j = 0; j < c; j++) total = total.dbl();
        for (auto &b : buckets) b = X::inf();
        const int bit = w * c;
        for (size_t i = 0; i < n; i++) {
            const uint32_t *r = &raw[8 * i];
            uint64_t two = (uint64_t)r[bit >> 5] | ((bit >> 5) + 1 < 8 ? (uint64_t)r[(bit >> 5) + 1] << 32 : 0);
            uint32_t d = (uint32_t)(two >> (bit & 31)) & ((1u << c) - 1);
            if (d) buckets[d - 1].madd(bases[i]);
        }
        X run = X::inf(), sum = X::inf();
        for (size_t d = buckets.size(); d-- > 0;) { run.add(buckets[d]); sum.add(run); }
        total.add(sum);
    }
    return total;
}

struct HostBatchBackend : BatchBackend {
    std::vector<G1A> bases;      // np x VB_OWN own points, then VB_SHARED per key
    size_t np = 0, nkeys = 1;
    void decompress(const G1Compressed *pts, size_t n, G1A *out, uint8_t *status) override {
        for (size_t i = 0; i < n; i++) status[i] = g1_decompress_check(sqrt_consts(), pts[i].x, pts[i].y_gt != 0, out[i]);
    }
    void public_input_eval(int lg_m, const Fr *betas, const uint8_t *bits, size_t n, size_t n_bits, Fr *out) override {
        for (size_t i = 0; i < n; i++) out[i] = host_public_input_eval(lg_m, betas[i], bits + i * n_bits, n_bits);
    }
    void public_input_eval_keyed(const int *lg_m, const size_t *n_bits, size_t, const uint32_t *key_of, const Fr *betas, const uint8_t *bits, const size_t *row_off, size_t n, Fr *out) override {
        for (size_t i = 0; i < n; i++) out[i] = host_public_input_eval(lg_m[key_of[i]], betas[i], bits + row_off[i], n_bits[key_of[i]]);
    }
    void set_bases(const G1A *own, size_t np_, const G1A *shared) override { set_bases_keyed(own, np_, shared, 1); }
    void set_bases_keyed(const G1A *own, size_t np_, const G1A *shared, size_t n_keys) override {
        np = np_; nkeys = n_keys;
        bases.assign(own, own + np * VB_OWN);
        bases.insert(bases.end(), shared, shared + nkeys * VB_SHARED);
    }
    XYZZ<Fq377> msm_main(const Fr *own_scalars, size_t lo, size_t hi, const Fr *shared_scalars) override {
        XYZZ<Fq377> r = host_msm(&bases[lo * VB_OWN], own_scalars + lo * VB_OWN, (hi - lo) * VB_OWN, Fr::BITS);
        r.add(host_msm(&bases[np * VB_OWN], shared_scalars, nkeys * VB_SHARED, Fr::BITS));
        return r;
    }
    XYZZ<Fq377> msm_w(const Fr *w_scalars, size_t lo, size_t hi) override {
        std::vector<G1A> w(2 * (hi - lo));
        for (size_t i = lo; i < hi; i++) { w[2 * (i - lo)] = bases[i * VB_OWN + S_WB]; w[2 * (i - lo) + 1] = bases[i * VB_OWN + S_WG]; }
        return host_msm(w.data(), w_scalars + 2 * lo, w.size(), 128);
    }
};
}  // namespace
std::unique_ptr<BatchBackend> make_host_batch_backend() { return std::unique_ptr<BatchBackend>(new HostBatchBackend()); }

std::vector<uint8_t> verify_batch(const VerifyingKey &vk, const uint8_t *proofs, const size_t *proof_lens, size_t n, const uint8_t *bits, size_t n_bits, BatchBackend &be,
                                  BatchTimings *timings) {
    BatchTimings T;
    const auto t_all = Clock::now();
    std::vector<uint8_t> accepted(n, 0);
    const size_t m = next_pow2(n_bits + 1);
    if (m != vk.num_instance) { if (timings) *timings = T; return accepted; }      // InvalidPublicInputLength / the instance does not match the index: every proof rejected
    const size_t nh = next_pow2(vk.num_constraints), nk = next_pow2(vk.num_non_zero);
    // ---- parse; the points stay compressed
    auto t0 = Clock::now();
    std::vector<size_t> offs(n + 1, 0);
    for (size_t i = 0; i < n; i++) offs[i + 1] = offs[i] + proof_lens[i];
    std::vector<RawProof> raw(n);
    std::vector<size_t> alive;               // proofs still in the batch
    for (size_t i = 0; i < n; i++) if (parse_raw_proof(proofs + offs[i], proof_lens[i], raw[i])) alive.push_back(i);
    T.parse_ms = ms_since(t0);
    // ---- decompression and subgroup checks, every point of every parsed proof in one call
    t0 = Clock::now();
    std::vector<G1A> own;                    // alive.size() x VB_OWN
    {
        std::vector<G1Compressed> todo;
        std::vector<size_t> where;
        for (size_t a = 0; a < alive.size(); a++) for (size_t s = 0; s < VB_OWN; s++) if (!raw[alive[a]].inf[s]) { todo.push_back(raw[alive[a]].pts[s]); where.push_back(a * VB_OWN + s); }
        std::vector<G1A> pts(todo.size() ? todo.size() : 1);
        std::vector<uint8_t> st(todo.size() ? todo.size() : 1, 0);
        if (!todo.empty()) be.decompress(todo.data(), todo.size(), pts.data(), st.data());
        std::vector<G1A> all(alive.size() * VB_OWN, G1A::inf());
        std::vector<uint8_t> bad(alive.size(), 0);
        for (size_t j = 0; j < todo.size(); j++) { if (st[j] != G1_OK) bad[where[j] / VB_OWN] = 1; else all[where[j]] = pts[j]; }
        std::vector<size_t> keep;
        for (size_t a = 0; a < alive.size(); a++) if (!bad[a]) { keep.push_back(alive[a]); own.insert(own.end(), all.begin() + a * VB_OWN, all.begin() + (a + 1) * VB_OWN); }
        alive.swap(keep);
    }
    T.decompress_ms = ms_since(t0);
    const size_t np = alive.size();
    if (np == 0) { T.total_ms = ms_since(t_all); if (timings) *timings = T; return accepted; }
    // ---- transcripts
    t0 = Clock::now();
    const Bytes prefix = transcript_prefix(vk);
    std::vector<Challenges> ch(np);
    std::vector<Fr> betas(np);
    std::vector<uint8_t> rows_bits(np * (n_bits ? n_bits : 1));
    for (size_t a = 0; a < np; a++) {
        const uint8_t *b = bits + alive[a] * n_bits;
        if (n_bits) memcpy(&rows_bits[a * n_bits], b, n_bits);
        ch[a] = run_transcript(prefix, nh, m, b, n_bits, &own[a * VB_OWN], raw[alive[a]].evals);
        betas[a] = ch[a].beta;
    }
    T.transcripts_ms = ms_since(t0);
    // ---- x^(beta_i)
    t0 = Clock::now();
    std::vector<Fr> xhat(np);
    be.public_input_eval(log2_exact(m), betas.data(), rows_bits.data(), np, n_bits, xhat.data());
    T.xhat_ms = ms_since(t0);
    // ---- randomizers: ChaCha20 keyed with SHA-256 over the key, the batch size and every proof with its public input -- fixed only once the whole batch is
    t0 = Clock::now();
    ChaChaRng rrng;
    {
        Bytes d;
        static const char domain[] = "zkaes verify_batch v1";
        d.put(domain, sizeof domain);
        std::vector<uint8_t> ark = serialize_vk_ark(vk);
        d.u64(ark.size()); d.put(ark.data(), ark.size());
        d.u64(n); d.u64(n_bits);
        for (size_t i = 0; i < n; i++) {
            d.u64(proof_lens[i]); d.put(proofs + offs[i], proof_lens[i]);
            for (size_t j = 0; j < n_bits; j++) d.u8(bits[i * n_bits + j] ? 1 : 0);
        }
        const size_t whole = d.b.size() / 64 * 64;
        uint8_t h[32], seed[32];
        sha256_chain(nullptr, d.b.data(), whole, h);
        sha256_finish(h, whole, d.b.data() + whole, d.b.size() - whole, seed);
        rrng.reseed(seed, 20);
    }
    auto draw128 = [&]() {
        for (;;) {
            uint64_t lo = rrng.next_u64(), hi = rrng.next_u64();
            if (!(lo | hi)) continue;          // a zero weight would take its equation out of the check
            uint32_t r[8] = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32), 0, 0, 0, 0};
            return Fr::from_raw(r);
        }
    };
    std::vector<Fr> rnd(2 * n);               // drawn for every proof of the call, in order, whether it is still in the batch or not
    for (auto &r : rnd) r = draw128();
    std::vector<Fr> own_sc(np * VB_OWN), w_sc(2 * np);
    std::vector<Rows> rows(np);
    for (size_t a = 0; a < np; a++) {
        const size_t i = alive[a];
        rows[a] = scalar_rows(vk, nh, m, nk, ch[a], xhat[a], raw[i].evals, raw[i].random_v_beta, rnd[2 * i], rnd[2 * i + 1]);
        for (size_t s = 0; s < VB_OWN; s++) own_sc[a * VB_OWN + s] = rows[a].own[s];
        w_sc[2 * a] = rows[a].w[0]; w_sc[2 * a + 1] = rows[a].w[1];
    }
    T.transcripts_ms += ms_since(t0);
    G1A shared[VB_SHARED];
    for (int i = 0; i < 6; i++) shared[K_IX + i] = vk.index_comms[i];
    shared[K_SP] = vk.shift_powers[0]; shared[K_SP + 1] = vk.shift_powers[1]; shared[K_G] = vk.g; shared[K_GG] = vk.gamma_g;
    t0 = Clock::now();
    be.set_bases(own.data(), np, shared);
    T.msm_ms += ms_since(t0);
    // ---- the batch equation over proofs [lo, hi) of the survivors
    auto holds = [&](size_t lo, size_t hi) {
        auto t1 = Clock::now();
        Fr sh[VB_SHARED];
        for (auto &v : sh) v = Fr::zero();
        for (size_t a = lo; a < hi; a++) for (size_t s = 0; s < VB_SHARED; s++) sh[s] = sh[s] + rows[a].shared[s];
        XYZZ<Fq377> total_c = be.msm_main(own_sc.data(), lo, hi, sh), total_w = be.msm_w(w_sc.data(), lo, hi);
        T.msm_ms += ms_since(t1);
        t1 = Clock::now();
        G1A Ps[2] = {total_w.neg().to_affine(), total_c.to_affine()};
        pairing::G2Affine Qs[2] = {vk.beta_h, vk.h};
        bool ok = pairing::pairing_product_is_one(Ps, Qs, 2);
        T.pairing_ms += ms_since(t1);
        T.sub_batches++;
        return ok;
    };
    // bisection: a range that holds is accepted whole; one that fails is halved, and a lone proof's answer is its own two equations under its own randomizers.
    // When the left half of a failing range holds, the right half is known to fail and is not checked again as a whole
    std::function<bool(size_t, size_t, bool)> solve = [&](size_t lo, size_t hi, bool known_bad) {
        if (!known_bad && holds(lo, hi)) { for (size_t a = lo; a < hi; a++) accepted[alive[a]] = 1; return true; }
        if (hi - lo == 1) return false;
        const size_t mid = lo + (hi - lo) / 2;
        const bool left = solve(lo, mid, false);
        solve(mid, hi, left);
        return false;
    };
    solve(0, np, false);
    T.total_ms = ms_since(t_all);
    if (timings) *timings = T;
    return accepted;
}

// verify_batch over proofs of several keys.  kzg_setup_points draws beta, g, gamma_g and h from one fixed stream whatever the SRS size, so the keys of this
// library share g, gamma_g, h and beta_h, and the batch equation holds over proofs of different keys with every key's index commitments and shift powers as further
// bases.  Per key: the transcript prefix, scalar_rows' sizes and the domain X of x^(beta).  The stages, the bisection and the timings are verify_batch's
std::vector<uint8_t> verify_batch_keys(const VerifyingKey *const *vks, size_t n_keys, const uint32_t *key_of, const uint8_t *proofs, const size_t *proof_lens, size_t n, const uint8_t *bits,
                                       const size_t *n_bits_each, BatchBackend &be, BatchTimings *timings) {
    BatchTimings T;
    const auto t_all = Clock::now();
    if (n_keys == 0) throw std::invalid_argument("verify_batch_keys: at least one verifying key");
    if (n_keys > ((size_t)1 << 16)) throw std::invalid_argument("verify_batch_keys: at most 65536 verifying keys");
    for (size_t i = 0; i < n; i++) if (key_of[i] >= n_keys) throw std::invalid_argument("verify_batch_keys: proof " + std::to_string(i) + " names key " + std::to_string(key_of[i]) + " of " + std::to_string(n_keys));
    auto same_g2 = [](const pairing::G2Affine &a, const pairing::G2Affine &b) { return a.inf == b.inf && a.x == b.x && a.y == b.y; };
    auto same_g1 = [](const G1A &a, const G1A &b) { return a.x == b.x && a.y == b.y; };
    for (size_t k = 1; k < n_keys; k++)
        if (!same_g1(vks[k]->g, vks[0]->g) || !same_g1(vks[k]->gamma_g, vks[0]->gamma_g) || !same_g2(vks[k]->h, vks[0]->h) || !same_g2(vks[k]->beta_h, vks[0]->beta_h))
            throw std::invalid_argument("verify_batch_keys: the keys do not share one setup (g, gamma_g, h and beta_h of key " + std::to_string(k) + " differ from key 0's)");
    std::vector<uint8_t> accepted(n, 0);
    std::vector<size_t> nh(n_keys), nk(n_keys), mk(n_keys), kbits(n_keys);      // per key: |H|, |K|, |X| and the row length the back end evaluates (|X| - 1)
    std::vector<int> lgm(n_keys);
    for (size_t k = 0; k < n_keys; k++) {
        nh[k] = next_pow2(vks[k]->num_constraints); nk[k] = next_pow2(vks[k]->num_non_zero); mk[k] = vks[k]->num_instance;
        if (mk[k] == 0 || (mk[k] & (mk[k] - 1))) mk[k] = 0;                      // |X| no power of two: no row pads to it, every proof of the key is rejected
    }
    // ---- parse; the points stay compressed.  A row that does not pad to its own key's |X| rejects its proof alone
    auto t0 = Clock::now();
    std::vector<size_t> offs(n + 1, 0), roffs(n + 1, 0);
    for (size_t i = 0; i < n; i++) { offs[i + 1] = offs[i] + proof_lens[i]; roffs[i + 1] = roffs[i] + n_bits_each[i]; }
    std::vector<RawProof> raw(n);
    std::vector<size_t> alive;
    for (size_t i = 0; i < n; i++) {
        if (n_bits_each[i] >= ((size_t)1 << 46) || next_pow2(n_bits_each[i] + 1) != mk[key_of[i]]) continue;
        if (parse_raw_proof(proofs + offs[i], proof_lens[i], raw[i])) alive.push_back(i);
    }
    T.parse_ms = ms_since(t0);
    // ---- decompression and subgroup checks, every point of every parsed proof in one call
    t0 = Clock::now();
    std::vector<G1A> own;
    {
        std::vector<G1Compressed> todo;
        std::vector<size_t> where;
        for (size_t a = 0; a < alive.size(); a++) for (size_t s = 0; s < VB_OWN; s++) if (!raw[alive[a]].inf[s]) { todo.push_back(raw[alive[a]].pts[s]); where.push_back(a * VB_OWN + s); }
        std::vector<G1A> pts(todo.size() ? todo.size() : 1);
        std::vector<uint8_t> st(todo.size() ? todo.size() : 1, 0);
        if (!todo.empty()) be.decompress(todo.data(), todo.size(), pts.data(), st.data());
        std::vector<G1A> all(alive.size() * VB_OWN, G1A::inf());
        std::vector<uint8_t> bad(alive.size(), 0);
        for (size_t j = 0; j < todo.size(); j++) { if (st[j] != G1_OK) bad[where[j] / VB_OWN] = 1; else all[where[j]] = pts[j]; }
        std::vector<size_t> keep;
        for (size_t a = 0; a < alive.size(); a++) if (!bad[a]) { keep.push_back(alive[a]); own.insert(own.end(), all.begin() + a * VB_OWN, all.begin() + (a + 1) * VB_OWN); }
        alive.swap(keep);
    }
    T.decompress_ms = ms_since(t0);
    const size_t np = alive.size();
    if (np == 0) { T.total_ms = ms_since(t_all); if (timings) *timings = T; return accepted; }
    // ---- transcripts: one prefix per key, the proof's own key's sizes
    t0 = Clock::now();
    std::vector<Bytes> prefix(n_keys);
    std::vector<uint8_t> have_prefix(n_keys, 0);
    std::vector<Challenges> ch(np);
    std::vector<Fr> betas(np);
    std::vector<uint32_t> akey(np);
    std::vector<size_t> arow(np);             // where the survivor's row starts in the caller's bits
    for (size_t a = 0; a < np; a++) {
        const size_t i = alive[a], k = key_of[i];
        if (!have_prefix[k]) { prefix[k] = transcript_prefix(*vks[k]); have_prefix[k] = 1; }
        akey[a] = (uint32_t)k; arow[a] = roffs[i];
        ch[a] = run_transcript(prefix[k], nh[k], mk[k], bits + roffs[i], n_bits_each[i], &own[a * VB_OWN], raw[i].evals);
        betas[a] = ch[a].beta;
    }
    T.transcripts_ms = ms_since(t0);
    // ---- x^(beta_i), every proof over its own key's X.  The back end takes ONE row length per key: rows are handed over zero-padded to |X| - 1, the same statement
    t0 = Clock::now();
    std::vector<Fr> xhat(np);
    {
        std::vector<size_t> prow(np);
        size_t total = 0;
        for (size_t k = 0; k < n_keys; k++) { lgm[k] = mk[k] ? log2_exact(mk[k]) : 0; kbits[k] = mk[k] ? mk[k] - 1 : 0; }
        for (size_t a = 0; a < np; a++) { prow[a] = total; total += kbits[akey[a]]; }
        std::vector<uint8_t> padded(total ? total : 1, 0);
        for (size_t a = 0; a < np; a++) { const size_t nb = n_bits_each[alive[a]]; if (nb) memcpy(&padded[prow[a]], bits + arow[a], nb); }
        be.public_input_eval_keyed(lgm.data(), kbits.data(), n_keys, akey.data(), betas.data(), padded.data(), prow.data(), np, xhat.data());
    }
    T.xhat_ms = ms_since(t0);
    // ---- randomizers: as verify_batch's, over every key and every proof with its key index and its row
    t0 = Clock::now();
    ChaChaRng rrng;
    {
        Bytes d;
        static const char domain[] = "zkaes verify_batch_keys v1";
        d.put(domain, sizeof domain);
        d.u64(n_keys);
        for (size_t k = 0; k < n_keys; k++) { std::vector<uint8_t> ark = serialize_vk_ark(*vks[k]); d.u64(ark.size()); d.put(ark.data(), ark.size()); }
        d.u64(n);
        for (size_t i = 0; i < n; i++) {
            d.u64(key_of[i]); d.u64(n_bits_each[i]);
            d.u64(proof_lens[i]); d.put(proofs + offs[i], proof_lens[i]);
            for (size_t j = 0; j < n_bits_each[i]; j++) d.u8(bits[roffs[i] + j] ? 1 : 0);
        }
        const size_t whole = d.b.size() / 64 * 64;
        uint8_t h[32], seed[32];
        sha256_chain(nullptr, d.b.data(), whole, h);
        sha256_finish(h, whole, d.b.data() + whole, d.b.size() - whole, seed);
        rrng.reseed(seed, 20);
    }
    auto draw128 = [&]() {
        for (;;) {
            uint64_t lo = rrng.next_u64(), hi = rrng.next_u64();
            if (!(lo | hi)) continue;          // a zero weight would take its equation out of the check
            uint32_t r[8] = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32), 0, 0, 0, 0};
            return Fr::from_raw(r);
        }
    };
    std::vector<Fr> rnd(2 * n);               // drawn for every proof of the call, in order, whether it is still in the batch or not
    for (auto &r : rnd) r = draw128();
    std::vector<Fr> own_sc(np * VB_OWN), w_sc(2 * np);
    std::vector<Rows> rows(np);
    for (size_t a = 0; a < np; a++) {
        const size_t i = alive[a], k = akey[a];
        rows[a] = scalar_rows(*vks[k], nh[k], mk[k], nk[k], ch[a], xhat[a], raw[i].evals, raw[i].random_v_beta, rnd[2 * i], rnd[2 * i + 1]);
        for (size_t s = 0; s < VB_OWN; s++) own_sc[a * VB_OWN + s] = rows[a].own[s];
        w_sc[2 * a] = rows[a].w[0]; w_sc[2 * a + 1] = rows[a].w[1];
    }
    T.transcripts_ms += ms_since(t0);
    std::vector<G1A> shared(n_keys * VB_SHARED);
    for (size_t k = 0; k < n_keys; k++) {
        G1A *sk = &shared[k * VB_SHARED];
        for (int i = 0; i < 6; i++) sk[K_IX + i] = vks[k]->index_comms[i];
        sk[K_SP] = vks[k]->shift_powers[0]; sk[K_SP + 1] = vks[k]->shift_powers[1]; sk[K_G] = vks[k]->g; sk[K_GG] = vks[k]->gamma_g;
    }
    t0 = Clock::now();
    be.set_bases_keyed(own.data(), np, shared.data(), n_keys);
    T.msm_ms += ms_since(t0);
    // ---- the batch equation over proofs [lo, hi) of the survivors: every proof's shared scalars go into its own key's slot
    std::vector<Fr> sh(n_keys * VB_SHARED);
    auto holds = [&](size_t lo, size_t hi) {
        auto t1 = Clock::now();
        for (auto &v : sh) v = Fr::zero();
        for (size_t a = lo; a < hi; a++) for (size_t s = 0; s < VB_SHARED; s++) sh[akey[a] * VB_SHARED + s] = sh[akey[a] * VB_SHARED + s] + rows[a].shared[s];
        XYZZ<Fq377> total_c = be.msm_main(own_sc.data(), lo, hi, sh.data()), total_w = be.msm_w(w_sc.data(), lo, hi);
        T.msm_ms += ms_since(t1);
        t1 = Clock::now();
        G1A Ps[2] = {total_w.neg().to_affine(), total_c.to_affine()};
        pairing::G2Affine Qs[2] = {vks[0]->beta_h, vks[0]->h};
        bool ok = pairing::pairing_product_is_one(Ps, Qs, 2);
        T.pairing_ms += ms_since(t1);
        T.sub_batches++;
        return ok;
    };
    std::function<bool(size_t, size_t, bool)> solve = [&](size_t lo, size_t hi, bool known_bad) {
        if (!known_bad && holds(lo, hi)) { for (size_t a = lo; a < hi; a++) accepted[alive[a]] = 1; return true; }
        if (hi - lo == 1) return false;
        const size_t mid = lo + (hi - lo) / 2;
        const bool left = solve(lo, mid, false);
        solve(mid, hi, left);
        return false;
    };
    solve(0, np, false);
    T.total_ms = ms_since(t_all);
    if (timings) *timings = T;
    return accepted;
}

}  // namespace zk
