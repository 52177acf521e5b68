// csrc/circuit.cpp -- see circuit.hpp.  Host-only C++; no device code.
#if defined(__GNUC__) && !defined(__clang__)
// The compilers make a million small allocations here (one LC per constraint).  A g++ build under AddressSanitizer records the caller's stack at every one of them by
// walking frame pointers; without frame pointers it walks garbage, no two allocations share a stack, and the sanitizer's stack depot turns the compile quadratic
// (tests/cbc_trace_emu.cpp builds this file with -O2 -fsanitize=address and nothing else).  Ahead of the includes, so that the vector code instantiated here has them too.
#pragma GCC optimize("no-omit-frame-pointer")
#endif
#include "circuit.hpp"
#include <algorithm>
#include <array>
#include <stdexcept>
#include "trace_layout.h"

namespace zk {
namespace {

constexpr uint32_t WIT = 1u << 28;   // variable ids: 0 = One, i = Instance(i), WIT + j = Witness(j)  (ark Variable order)

// ---- Boolean literal: constant, or variable with optional negation (ark-r1cs-std Boolean::{Constant, Is, Not})
struct Bit {
    int32_t v;
    static Bit konst(bool b) { return Bit{b ? -1 : -2}; }
    static Bit is(uint32_t var) { return Bit{(int32_t)(var << 1)}; }
    bool is_const() const { return v < 0; }
    bool cval() const { return v == -1; }
    bool neg() const { return v & 1; }
    uint32_t var() const { return (uint32_t)v >> 1; }
    Bit operator!() const { return is_const() ? konst(!cval()) : Bit{v ^ 1}; }
};
using Byte = std::array<Bit, 8>;    // LSB first
using Word = std::array<Bit, 32>;

// ---- sorted sparse linear combination (ark-relations LinearCombination: sorted by Variable, duplicates merged)
struct LC {
    std::vector<std::pair<uint32_t, int64_t>> t;
    void add(int64_t c, uint32_t var) {
        auto it = std::lower_bound(t.begin(), t.end(), var, [](const std::pair<uint32_t, int64_t> &a, uint32_t b) { return a.first < b; });
        if (it != t.end() && it->first == var) it->second += c; else t.insert(it, {var, c});
    }
    void add(int64_t c, Bit b) {           // c * lc(b)
        if (b.is_const()) { if (b.cval()) add(c, 0u); }
        else if (!b.neg()) add(c, b.var());
        else { add(c, 0u); add(-c, b.var()); }
    }
};

struct RawMatrix {
    std::vector<uint32_t> rowptr{0};
    std::vector<uint32_t> var;
    std::vector<int64_t> coeff;
    void push(const LC &l) {
        for (auto &e : l.t) if (e.second != 0) { var.push_back(e.first); coeff.push_back(e.second); }   // make_row drops zero coefficients
        rowptr.push_back((uint32_t)var.size());
    }
};

class Builder {
  public:
    RawMatrix A, B, C;
    uint32_t n_instance = 1;              // Variable::One
    uint32_t n_witness = 0;
    std::vector<uint32_t> inst_desc{(WD_CONST << WD_KIND_SHIFT) | 1u};
    std::vector<uint32_t> wit_desc;
    std::vector<uint32_t> sbox_tmpl, sbox_in_off;

    uint32_t new_witness() { wit_desc.push_back(0xffffffffu); return WIT + n_witness++; }
    uint32_t new_input() { inst_desc.push_back(0xffffffffu); return n_instance++; }
    void enforce(const LC &a, const LC &b, const LC &c) { A.push(a); B.push(b); C.push(c); }
    void set_desc(uint32_t var, uint32_t d) { (var >= WIT ? wit_desc[var - WIT] : inst_desc[var]) = d; }
    // tag the variable behind `b` (if it was created at or after witness watermark `mark`) with a trace bit
    void tag_bytebit(Bit b, uint32_t mark, uint32_t off, int bit) {
        if (b.is_const() || b.var() < WIT + mark) return;
        set_desc(b.var(), (WD_BYTEBIT << WD_KIND_SHIFT) | (off << 4) | ((uint32_t)bit << 1) | (b.neg() ? 1u : 0u));
    }

    // AllocatedBool::new_variable: (1 - a) * a = 0
    Bit alloc(bool input, uint32_t off, int bit) {
        uint32_t v = input ? new_input() : new_witness();
        LC a, b, c;
        a.add(1, 0u); a.add(-1, v); b.add(1, v);
        enforce(a, b, c);
        set_desc(v, (WD_BYTEBIT << WD_KIND_SHIFT) | (off << 4) | ((uint32_t)bit << 1));
        return Bit::is(v);
    }
    uint32_t raw_xor(uint32_t a, uint32_t b) {        // (a + a) * b = a + b - c
        uint32_t r = new_witness();
        LC A_, B_, C_;
        A_.add(1, a); A_.add(1, a); B_.add(1, b); C_.add(1, a); C_.add(1, b); C_.add(-1, r);
        enforce(A_, B_, C_);
        return r;
    }
    Bit bxor(Bit a, Bit b) {
        if (a.is_const()) return a.cval() ? !b : b;
        if (b.is_const()) return b.cval() ? !a : a;
        if (a.neg() != b.neg()) { Bit is = a.neg() ? b : a, nt = a.neg() ? a : b; return !Bit::is(raw_xor(is.var(), nt.var())); }
        return Bit::is(raw_xor(a.var(), b.var()));
    }
    Bit band(Bit a, Bit b) {
        if (a.is_const()) return a.cval() ? b : Bit::konst(false);
        if (b.is_const()) return b.cval() ? a : Bit::konst(false);
        LC A_, B_, C_;
        if (!a.neg() && !b.neg()) { A_.add(1, a.var()); B_.add(1, b.var()); }                       // and
        else if (a.neg() && b.neg()) { A_.add(1, 0u); A_.add(-1, a.var()); B_.add(1, 0u); B_.add(-1, b.var()); }   // nor
        else { Bit is = a.neg() ? b : a, nt = a.neg() ? a : b; A_.add(1, is.var()); B_.add(1, 0u); B_.add(-1, nt.var()); }   // and_not
        uint32_t r = new_witness();
        C_.add(1, r);
        enforce(A_, B_, C_);
        return Bit::is(r);
    }
    Bit bor(Bit a, Bit b) {
        if (a.is_const()) return a.cval() ? Bit::konst(true) : b;
        if (b.is_const()) return b.cval() ? Bit::konst(true) : a;
        if (!a.neg() && !b.neg()) {                     // (1-a) * (1-b) = (1-c)
            uint32_t r = new_witness();
            LC A_, B_, C_;
            A_.add(1, 0u); A_.add(-1, a.var()); B_.add(1, 0u); B_.add(-1, b.var()); C_.add(1, 0u); C_.add(-1, r);
            enforce(A_, B_, C_);
            return Bit::is(r);
        }
        if (a.neg() && b.neg()) return !band(!b, !a);   // (b @ Not, a @ Not) => a.not().and(b.not()).not() with a = second operand
        Bit is = a.neg() ? b : a, nt = a.neg() ? a : b;
        return !band(!is, !nt);
    }
    Bit select(Bit cond, Bit t, Bit f) {
        if (cond.is_const()) return cond.cval() ? t : f;
        if (cond.neg()) return select(!cond, f, t);
        if (f.is_const() && !f.cval()) return band(cond, t);
        if (t.is_const() && !t.cval()) return band(!cond, f);
        if (t.is_const() && t.cval()) return bor(cond, f);
        if (f.is_const() && f.cval()) return bor(!cond, t);
        uint32_t r = new_witness();                     // cond * (t - f) = r - f
        LC A_, B_, C_;
        A_.add(1, cond); B_.add(1, t); B_.add(-1, f); C_.add(1, r); C_.add(-1, f);
        enforce(A_, B_, C_);
        return Bit::is(r);
    }
    void enforce_equal(Bit self, Bit other) {           // difference * 1 = 0
        if (self.is_const() && other.is_const()) return;
        LC d, one, z;
        if (self.is_const() || other.is_const()) {
            Bit c = self.is_const() ? self : other, x = self.is_const() ? other : self;
            bool one_minus = (c.cval() && !x.neg()) || (!c.cval() && x.neg());
            if (one_minus) { d.add(1, 0u); d.add(-1, x.var()); } else d.add(1, x.var());
        } else if (!self.neg() && !other.neg()) { d.add(1, other.var()); d.add(-1, self.var()); }
        else if (self.neg() && other.neg()) { d.add(1, self.var()); d.add(-1, other.var()); }
        else { Bit is = self.neg() ? other : self, nt = self.neg() ? self : other; d.add(1, 0u); d.add(-1, nt.var()); d.add(-1, is.var()); }
        one.add(1, 0u);
        enforce(d, one, z);
    }

    // ---- bytes / words
    static Byte const_byte(uint8_t v) { Byte r; for (int i = 0; i < 8; i++) r[i] = Bit::konst((v >> i) & 1); return r; }
    Byte alloc_byte(bool input, uint32_t off) { Byte r; for (int i = 0; i < 8; i++) r[i] = alloc(input, off, i); return r; }
    // xor whose result byte lives at trace offset `off`
    Byte xor_byte(const Byte &a, const Byte &b, uint32_t off) {
        Byte r;
        for (int i = 0; i < 8; i++) { uint32_t mark = n_witness; r[i] = bxor(a[i], b[i]); tag_bytebit(r[i], mark, off, i); }
        return r;
    }
    static Byte shl(const Byte &a, int n) { Byte r; for (int i = 0; i < 8; i++) r[i] = i >= n ? a[i - n] : Bit::konst(false); return r; }
    static Byte shr(const Byte &a, int n) { Byte r; for (int i = 0; i < 8; i++) r[i] = i + n < 8 ? a[i + n] : Bit::konst(false); return r; }

    // UInt8::conditionally_select_power_of_two_vector over the constant S-box table (src/aes_circuit.rs:243-248)
    Byte sbox(const Byte &x, const std::vector<Byte> &table, uint32_t in_off) {
        uint32_t inst = (uint32_t)sbox_in_off.size();
        sbox_in_off.push_back(in_off);
        bool record = sbox_tmpl.empty();
        uint32_t tix = 0;
        std::vector<Byte> cur(table), nxt;
        for (int lvl = 0; lvl < 8; lvl++) {
            nxt.assign(cur.size() / 2, Byte{});
            for (size_t j = 0; j < cur.size(); j += 2)
                for (int k = 0; k < 8; k++) {
                    uint32_t mark = n_witness;
                    Bit r = select(x[lvl], cur[j + 1][k], cur[j][k]);
                    nxt[j / 2][k] = r;
                    if (n_witness != mark) {
                        if (n_witness != mark + 1 || r.is_const() || r.var() != WIT + mark) throw std::logic_error("sbox: unexpected allocation pattern");
                        uint32_t entry = ((uint32_t)lvl << 12) | ((uint32_t)(j / 2) << 4) | ((uint32_t)k << 1);
                        if (record) sbox_tmpl.push_back(entry);
                        else if (tix >= sbox_tmpl.size() || sbox_tmpl[tix] != entry) throw std::logic_error("sbox: template differs between instances");
                        set_desc(r.var(), (WD_SBOX << WD_KIND_SHIFT) | (inst << 11) | (tix << 1) | (r.neg() ? 1u : 0u));
                        tix++;
                    }
                }
            cur.swap(nxt);
        }
        if (!record && tix != sbox_tmpl.size()) throw std::logic_error("sbox: template length differs");
        return cur[0];
    }
    // src/helpers/mod.rs:11-42
    Byte helpers_add(const Byte &augend, const Byte &addend) {
        Byte sum; Bit carry = Bit::konst(false);
        for (int i = 0; i < 8; i++) {
            Bit a = augend[i], b = addend[i];
            sum[i] = bxor(bxor(carry, a), b);
            carry = bor(band(!carry, band(a, b)), band(carry, bor(a, b)));
        }
        return sum;
    }
    // src/helpers/mod.rs:44-64 (multiplier is a constant here; the reference branches on its bit values)
    Byte helpers_multiply(const Byte &multiplicand, uint8_t multiplier) {
        Byte product = const_byte(0);
        for (int i = 0; i < 8; i++)
            if ((multiplier >> i) & 1) product = helpers_add(product, i ? shl(multiplicand, i) : multiplicand);
        return product;
    }
};

CsrMatrix finalize_matrix(const RawMatrix &m, uint32_t n_inst_padded, size_t rows_padded) {
    CsrMatrix o;
    o.rowptr = m.rowptr;
    o.rowptr.resize(rows_padded + 1, (uint32_t)m.var.size());
    o.col.resize(m.var.size());
    for (size_t i = 0; i < m.var.size(); i++) o.col[i] = m.var[i] < WIT ? m.var[i] : n_inst_padded + (m.var[i] - WIT);
    o.coeff = m.coeff;
    return o;
}

// ark-marlin padding (pad_input_for_indexer_and_prover + make_matrices_square) and final column numbering
Circuit finish(Builder &b, int kind, size_t n_blocks, size_t trace_bytes, size_t key_bytes = 16) {
    Circuit c;
    c.kind = kind; c.n_blocks = n_blocks; c.key_bytes = key_bytes; c.message_bytes = 16 * n_blocks; c.trace_bytes = trace_bytes;
    c.raw_constraints = b.A.rowptr.size() - 1; c.raw_instance = b.n_instance; c.raw_witness = b.n_witness;
    size_t ninst = 1;
    while (ninst < b.n_instance) ninst <<= 1;
    std::vector<uint32_t> desc(b.inst_desc);
    desc.resize(ninst, (WD_CONST << WD_KIND_SHIFT) | 0u);            // padded inputs are zero
    size_t nwit = b.n_witness, ncons = c.raw_constraints;
    if (ninst + nwit > ncons) ncons = ninst + nwit;                   // dummy 0*0=0 rows
    else nwit = ncons - ninst;                                        // dummy witnesses = F::one()
    desc.insert(desc.end(), b.wit_desc.begin(), b.wit_desc.end());
    desc.resize(ninst + nwit, (WD_CONST << WD_KIND_SHIFT) | 1u);
    for (uint32_t d : desc) if (d == 0xffffffffu) throw std::logic_error("circuit: variable without a witness descriptor");
    c.num_instance = ninst; c.num_witness = nwit; c.num_constraints = ncons;
    c.A = finalize_matrix(b.A, (uint32_t)ninst, ncons); c.B = finalize_matrix(b.B, (uint32_t)ninst, ncons); c.C = finalize_matrix(b.C, (uint32_t)ninst, ncons);
    c.desc.swap(desc);
    c.sbox_in_off = b.sbox_in_off; c.sbox_tmpl = b.sbox_tmpl;
    return c;
}

}  // namespace

uint8_t aes_sbox_value(uint8_t x) {   // algebraic S-box (FIPS-197 5.1.1; equals the 256 constants of src/aes_circuit.rs:433-694)
    auto mul = [](uint8_t a, uint8_t b) { uint8_t p = 0; for (int i = 0; i < 8; i++) { if (b & 1) p ^= a; bool h = a & 0x80; a <<= 1; if (h) a ^= 0x1B; b >>= 1; } return p; };
    uint8_t inv = 0;
    if (x) { inv = 1; for (int i = 0; i < 254; i++) inv = mul(inv, x); }
    uint8_t r = inv;
    for (int i = 1; i <= 4; i++) r ^= (uint8_t)((inv << i) | (inv >> (8 - i)));
    return r ^ 0x63;
}

namespace {

// The gates every AES mode shares, in the reference's order: the key schedule once, then per block the Nr rounds behind a round-0 input.  ECB feeds the message block,
// CBC the chained block X_b; everything a block allocates from its round 0 on is the same gate sequence in both.  nk = the key length in words (4, 6, 8): Nr = nk + 6
// rounds, 4 (Nr + 1) schedule words (FIPS-197 5.2), the trace laid out by the TRK_* macros of trace_layout.h; at nk = 4 every gate and every offset is the reference's.
struct AesGates {
    Builder &b;
    const int nk, nr;
    std::vector<Byte> table;
    std::vector<Byte> key;
    std::vector<std::array<Byte, 4>> w;
    AesGates(Builder &b_, size_t key_bits) : b(b_), nk((int)(key_bits / 32)), nr(nk + 6), table(256), key(4 * (size_t)nk), w(4 * ((size_t)nr + 1)) {
        for (int i = 0; i < 256; i++) table[i] = Builder::const_byte(aes_sbox_value((uint8_t)i));
    }
    size_t key_bytes() const { return 4 * (size_t)nk; }
    uint32_t blk(size_t bi) const { return (uint32_t)(TRK_BLOCK0(nk) + bi * TRK_BLOCK_STRIDE(nk)); }
    // message then key witnesses (src/lib.rs:70-76, 82-88)
    std::vector<Byte> alloc_message_and_key(size_t len) {
        std::vector<Byte> msg(len);
        for (size_t i = 0; i < len; i++) msg[i] = b.alloc_byte(false, blk(i / 16) + TR_BL_MSG + (uint32_t)(i % 16));
        for (int i = 0; i < 4 * nk; i++) key[i] = b.alloc_byte(false, TR_KEY + i);
        return msg;
    }
    // derive_keys (src/aes_circuit.rs:20-129): words are big-endian byte quadruples; UInt32::xor runs LSB-first over the
    // u32, i.e. byte 3 first (to_u32, :201-212).  FIPS-197 5.2 for any nk: W_i = W_{i-nk} ^ temp, temp = SubWord(RotWord(W_{i-1})) ^ Rcon at i % nk == 0,
    // SubWord(W_{i-1}) at i % nk == 4 when nk = 8, else W_{i-1}
    void key_schedule() {
        for (int i = 0; i < nk; i++) for (int k = 0; k < 4; k++) w[i][k] = key[4 * i + k];
        static const uint8_t rc[10] = {0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80, 0x1B, 0x36};
        for (int i = nk; i < 4 * (nr + 1); i++) {
            if (i % nk == 0) {
                int q = TRK_KS_INST_OF(nk, i);
                std::array<Byte, 4> sub;
                for (int k = 0; k < 4; k++) {
                    int src = (k + 1) % 4;                                            // rotate_word: rotate_left(1)
                    sub[k] = b.sbox(w[i - 1][src], table, (uint32_t)(TRK_KS_W(nk) + 4 * (i - 1) + src));
                }
                for (int k = 3; k >= 0; k--) w[i][k] = b.xor_byte(w[i - nk][k], sub[k], (uint32_t)(TRK_KS_PRE(nk) + 4 * q + k));
                w[i][0] = b.xor_byte(w[i][0], Builder::const_byte(rc[i / nk - 1]), 0);         // Rcon: constant operand, free
            } else if (nk == 8 && i % 8 == 4) {
                int q = TRK_KS_INST_OF(nk, i);                                        // no rotation, no Rcon: the word ahead of the (absent) Rcon xor is W_i itself
                std::array<Byte, 4> sub;
                for (int k = 0; k < 4; k++) sub[k] = b.sbox(w[i - 1][k], table, (uint32_t)(TRK_KS_W(nk) + 4 * (i - 1) + k));
                for (int k = 3; k >= 0; k--) w[i][k] = b.xor_byte(w[i - nk][k], sub[k], (uint32_t)(TRK_KS_PRE(nk) + 4 * q + k));
            } else {
                for (int k = 3; k >= 0; k--) w[i][k] = b.xor_byte(w[i - nk][k], w[i - 1][k], (uint32_t)(TRK_KS_W(nk) + 4 * i + k));
            }
        }
    }
    // one block's rounds (src/lib.rs:194-278) from its round-0 input `in`; returns S_Nr.  The block's slot is number bi behind TRK_BLOCK0, or lies at any trace base
    std::array<Byte, 16> block_rounds(const Byte *in, size_t bi) { return block_rounds_at(in, blk(bi)); }
    std::array<Byte, 16> block_rounds_at(const Byte *in, uint32_t base) {
        const uint32_t xt_off = TRK_BL_XT(nk), mp_off = TRK_BL_MP(nk);
        std::array<Byte, 16> s, t, u;
        for (int i = 0; i < 16; i++) s[i] = b.xor_byte(in[i], key[i], base + TR_BL_S + i);          // :196 raw key (round key 0 = the first 16 key bytes for every nk)
        for (int r = 1; r <= nr; r++) {
            for (int i = 0; i < 16; i++) {                                                                      // substitute_bytes
                t[i] = b.sbox(s[i], table, base + TR_BL_S + 16 * (r - 1) + i);
            }
            for (int c = 0; c < 4; c++) for (int rr = 0; rr < 4; rr++) u[4 * c + rr] = t[4 * ((c + rr) % 4) + rr];   // shift_rows
            if (r <= nr - 1) {                                                                                   // mix_columns
                for (int c = 0; c < 4; c++) {
                    std::array<Byte, 4> a{u[4 * c], u[4 * c + 1], u[4 * c + 2], u[4 * c + 3]}, xb;
                    for (int k = 0; k < 4; k++) {
                        Byte sh = Builder::shr(a[k], 7), h, one = Builder::const_byte(1);
                        for (int i = 0; i < 8; i++) h[i] = b.band(sh[i], one[i]);
                        Byte m = b.helpers_multiply(h, 0x1B);
                        xb[k] = b.xor_byte(Builder::shl(a[k], 1), m, base + xt_off + 16 * (r - 1) + 4 * c + k);
                    }
                    static const int order[4][5][2] = {{{1, 0}, {0, 3}, {0, 2}, {1, 1}, {0, 1}}, {{1, 1}, {0, 0}, {0, 3}, {1, 2}, {0, 2}},
                                                       {{1, 2}, {0, 1}, {0, 0}, {1, 3}, {0, 3}}, {{1, 3}, {0, 2}, {0, 1}, {1, 0}, {0, 0}}};
                    for (int o = 0; o < 4; o++) {
                        Byte acc = order[o][0][0] ? xb[order[o][0][1]] : a[order[o][0][1]];
                        for (int p = 1; p < 5; p++) {
                            const Byte &x = order[o][p][0] ? xb[order[o][p][1]] : a[order[o][p][1]];
                            acc = b.xor_byte(acc, x, base + mp_off + 64 * (r - 1) + 4 * (4 * c + o) + (p - 1));
                        }
                        t[4 * c + o] = acc;
                    }
                }
            } else {
                t = u;
            }
            for (int i = 0; i < 16; i++) {
                Byte rk;                                                          // round key r = words 4r..4r+3 as bytes
                rk = w[4 * r + i / 4][i % 4];
                s[i] = b.xor_byte(t[i], rk, base + TR_BL_S + 16 * r + i);
            }
        }
        return s;
    }
    // public inputs + equality (src/lib.rs:282-286)
    void ciphertext_inputs(const std::vector<Byte> &ct) {
        for (size_t i = 0; i < ct.size(); i++) {
            Byte pi = b.alloc_byte(true, blk(i / 16) + (uint32_t)TRK_BL_CT(nk) + (uint32_t)(i % 16));
            for (int k = 0; k < 8; k++) b.enforce_equal(pi[k], ct[i][k]);
        }
    }
    // The key tag, behind everything the mode emits: per tag block the rounds of the constant block D_t -- round 0 is constant ^ key and costs no gate, as for
    // GCM's H block; its S_0 bits are key bits, negated where D_t has a one -- in the slot at mode_bytes rounded up to 16 plus t strides, then 128 inputs equal to its S_Nr.
    // Returns the trace length with the slots
    size_t key_tag(size_t tag_blocks, size_t mode_bytes) {
        for (size_t t = 0; t < tag_blocks; t++) {
            const uint32_t base = (uint32_t)TRK_KT_SLOT(nk, mode_bytes, t);
            uint8_t d[16];
            aes_key_tag_block(t, d);
            std::array<Byte, 16> in;
            for (int i = 0; i < 16; i++) in[i] = Builder::const_byte(d[i]);
            const std::array<Byte, 16> s = block_rounds_at(in.data(), base);
            for (int i = 0; i < 16; i++) {
                Byte pi = b.alloc_byte(true, base + (uint32_t)TRK_BL_CT(nk) + (uint32_t)i);
                for (int k = 0; k < 8; k++) b.enforce_equal(pi[k], s[i][k]);
            }
        }
        return TRK_KT_BYTES(nk, mode_bytes, tag_blocks);
    }
};

// FIPS 180-4 4.2.2 and 5.3.3
const uint32_t SHA256_K[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
    0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
    0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
const uint32_t SHA256_IV[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};

// The SHA-256 compression function over the Builder's booleans.  A word is 32 Bits, bit i of weight 2^i; rotations and shifts are re-wirings.  Every xor and
// select result is tagged with its bit of the compression's trace slot (trace_layout.h TRD_*).  An addition mod 2^32 of n words (a constant counts as one) is 32 allocated
// result bits r_i, ceil(log2 n) allocated carry bits c_j and ONE row (sum_i 2^i operands - sum_i 2^i r_i - 2^32 sum_j 2^j c_j) * One = 0 with the difference in A, as in
// the GHASH parity rows.  The carry widths are 1, 2, 3, 3 bits for n = 2, 4, 6, 7 operands: the operands' sum stays below n 2^32 <= 7 2^32 and the right-hand side below
// 9 2^32, both far below the field's modulus r ~ 2^253, so the row holds over the integers, where result and carry of a sum are unique.  An addition whose operands are
// all constants (the schedule of a block that holds padding only) is a constant and costs nothing.
struct Sha256Gates {
    Builder &b;
    explicit Sha256Gates(Builder &b_) : b(b_) {}
    static Word const_word(uint32_t v) { Word r; for (int i = 0; i < 32; i++) r[i] = Bit::konst((v >> i) & 1); return r; }
    static Word rotr(const Word &x, int n) { Word r; for (int i = 0; i < 32; i++) r[i] = x[(i + n) % 32]; return r; }
    static Word shr(const Word &x, int n) { Word r; for (int i = 0; i < 32; i++) r[i] = i + n < 32 ? x[i + n] : Bit::konst(false); return r; }
    // word k of 4 big-endian bytes: bit i is bit i % 8 of byte 3 - i / 8
    static Word be_word(const Byte *bytes) { Word r; for (int i = 0; i < 32; i++) r[i] = bytes[3 - i / 8][i % 8]; return r; }
    Word xor_word(const Word &x, const Word &y, uint32_t off) {
        Word r;
        for (int i = 0; i < 32; i++) { uint32_t mark = b.n_witness; r[i] = b.bxor(x[i], y[i]); b.tag_bytebit(r[i], mark, off + (uint32_t)(i / 8), i % 8); }
        return r;
    }
    Word select_word(const Word &c, const Word &t, const Word &f, uint32_t off) {
        Word r;
        for (int i = 0; i < 32; i++) { uint32_t mark = b.n_witness; r[i] = b.select(c[i], t[i], f[i]); b.tag_bytebit(r[i], mark, off + (uint32_t)(i / 8), i % 8); }
        return r;
    }
    Word add(std::initializer_list<const Word *> ops, uint32_t konst, bool with_konst, int carry_bits, uint32_t off_r, uint32_t off_c) {
        bool all_const = true;
        for (const Word *w : ops) for (int i = 0; i < 32; i++) all_const = all_const && (*w)[i].is_const();
        if (all_const) {
            uint32_t v = with_konst ? konst : 0;
            for (const Word *w : ops) for (int i = 0; i < 32; i++) if ((*w)[i].cval()) v += 1u << i;
            return const_word(v);
        }
        LC d, one, z;
        for (const Word *w : ops) for (int i = 0; i < 32; i++) d.add((int64_t)1 << i, (*w)[i]);
        if (with_konst) d.add((int64_t)konst, 0u);
        Word r;
        for (int i = 0; i < 32; i++) { r[i] = b.alloc(false, off_r + (uint32_t)(i / 8), i % 8); d.add(-((int64_t)1 << i), r[i]); }
        for (int j = 0; j < carry_bits; j++) d.add(-((int64_t)1 << (32 + j)), b.alloc(false, off_c, j));
        one.add(1, 0u);
        b.enforce(d, one, z);
        return r;
    }
    // one compression from `st` (a .. h) over the block's 16 words, into the slot at trace offset `slot`; returns the feed-forward
    std::array<Word, 8> compress(const std::array<Word, 8> &st, const std::array<Word, 16> &block, uint32_t slot) {
        std::vector<Word> w(block.begin(), block.end());
        w.resize(64);
        for (int t = 16; t < 64; t++) {
            const uint32_t e = slot + TRD_SCH + (uint32_t)(TRD_SCH_STRIDE * (t - 16));
            const Word &x = w[t - 15], &y = w[t - 2];
            Word s0 = xor_word(xor_word(rotr(x, 7), rotr(x, 18), e + TRD_SCH_S0X), shr(x, 3), e + TRD_SCH_S0);
            Word s1 = xor_word(xor_word(rotr(y, 17), rotr(y, 19), e + TRD_SCH_S1X), shr(y, 10), e + TRD_SCH_S1);
            w[t] = add({&s1, &w[t - 7], &s0, &w[t - 16]}, 0, false, 2, e + TRD_SCH_W, e + TRD_SCH_CARRY);
        }
        Word a = st[0], bb = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
        for (int t = 0; t < 64; t++) {
            const uint32_t o = slot + TRD_RND + (uint32_t)(TRD_RND_STRIDE * t);
            Word S1 = xor_word(xor_word(rotr(e, 6), rotr(e, 11), o + TRD_RND_S1X), rotr(e, 25), o + TRD_RND_S1);
            Word ch = select_word(e, f, g, o + TRD_RND_CH);
            Word S0 = xor_word(xor_word(rotr(a, 2), rotr(a, 13), o + TRD_RND_S0X), rotr(a, 22), o + TRD_RND_S0);
            Word ab = xor_word(a, bb, o + TRD_RND_AB);
            Word maj = select_word(ab, c, a, o + TRD_RND_MAJ);
            Word e2 = add({&d, &h, &S1, &ch, &w[t]}, SHA256_K[t], true, 3, o + TRD_RND_E, o + TRD_RND_CE);
            Word a2 = add({&h, &S1, &ch, &w[t], &S0, &maj}, SHA256_K[t], true, 3, o + TRD_RND_A, o + TRD_RND_CA);
            h = g; g = f; f = e; e = e2; d = c; c = bb; bb = a; a = a2;
        }
        const Word out[8] = {a, bb, c, d, e, f, g, h};
        std::array<Word, 8> r;
        for (int k = 0; k < 8; k++) r[k] = add({&st[k], &out[k]}, 0, false, 1, slot + TRD_FF + 4 * (uint32_t)k, slot + TRD_FF + TRD_FF_CARRY + 4 * (uint32_t)k);
        return r;
    }
    // The whole digest part of a key, behind everything else it emits: 256 inputs H_in, the compressions over msg (and, for a final key, the padding constants), 256
    // inputs H_out equal to the last feed-forward.  Message word t of block j, bit i, is bit i % 8 of byte 64 j + 4 t + 3 - i / 8: a re-wiring of the message witnesses.
    // `bytes` = the trace length ahead of the region; returns the length with it
    // bits_input (the last segment of a GCM digest record; final keys only): the padding's eight length bytes are INPUTS, the big-endian bit count of
    // everything hashed, which the verifier sets; their trace bytes lie behind the region's slots (TRS_DG_BITS).  The 256 H_out inputs are then allocated ahead of them
    // and of the compressions, so that the instance reads H_in, H_out, total_bits; their equalities stay where they were
    size_t digest(const std::vector<Byte> &msg, int kind, uint64_t prefix, size_t bytes, bool bits_input = false) {
        const size_t len = msg.size(), nblk = TRD_BLOCKS(kind, len);
        const uint32_t dg = (uint32_t)TRD(bytes);
        std::vector<Byte> padded(msg);
        if (kind == DIGEST_FINAL) {
            padded.push_back(Builder::const_byte(0x80));
            padded.resize(64 * nblk, Builder::const_byte(0));
            const uint64_t bits = 8 * (prefix + (uint64_t)len);
            for (int i = 0; i < 8; i++) padded[64 * nblk - 8 + i] = Builder::const_byte((uint8_t)(bits >> (56 - 8 * i)));
        }
        std::array<Byte, 32> hin, hout;
        for (int j = 0; j < 32; j++) hin[j] = b.alloc_byte(true, dg + TRD_HIN + (uint32_t)j);
        if (bits_input) {
            for (int j = 0; j < 32; j++) hout[j] = b.alloc_byte(true, dg + TRD_HOUT + (uint32_t)j);
            for (int i = 0; i < 8; i++) padded[64 * nblk - 8 + i] = b.alloc_byte(true, dg + (uint32_t)TRS_DG_BITS(nblk) + (uint32_t)i);
        }
        std::array<Word, 8> st;
        for (int k = 0; k < 8; k++) st[k] = be_word(&hin[4 * k]);
        for (size_t j = 0; j < nblk; j++) {
            std::array<Word, 16> block;
            for (int t = 0; t < 16; t++) block[t] = be_word(&padded[64 * j + 4 * t]);
            st = compress(st, block, dg + TRD_SLOT0 + (uint32_t)(j * TRD_SLOT_STRIDE));
        }
        for (int j = 0; j < 32; j++) {
            Byte pi = bits_input ? hout[j] : b.alloc_byte(true, dg + TRD_HOUT + (uint32_t)j);
            for (int k = 0; k < 8; k++) b.enforce_equal(pi[k], st[j / 4][8 * (3 - j % 4) + k]);
        }
        return TRD_BYTES(bytes, kind, nblk) + (bits_input ? 16 : 0);
    }
};

}  // namespace

namespace {
void require_key_bits(size_t key_bits) {
    if (key_bits != 128 && key_bits != 192 && key_bits != 256) throw std::invalid_argument("the AES key size must be 128, 192 or 256 bits");
}
void require_key_tag_blocks(size_t key_tag_blocks) {
    if (key_tag_blocks > 2) throw std::invalid_argument("key_tag_blocks must be 0, 1 or 2");
}
// what every AES compiler checks about its digest arguments before it emits a gate
void require_digest(int digest_kind, uint64_t digest_prefix, size_t len) {
    if (digest_kind != DIGEST_NONE && digest_kind != DIGEST_CHAIN && digest_kind != DIGEST_FINAL) throw std::invalid_argument("digest_kind must be 0 (none), 1 (chain) or 2 (final)");
    if (digest_kind != DIGEST_FINAL && digest_prefix) throw std::invalid_argument("digest_prefix belongs to a final digest key only");
    if (digest_kind == DIGEST_CHAIN && (len == 0 || len % 64)) throw std::invalid_argument("a chain digest key takes a message of a non-zero multiple of 64 bytes");
    if (digest_kind == DIGEST_FINAL && (digest_prefix % 64 || digest_prefix >= ((uint64_t)1 << 61) || (uint64_t)len >= ((uint64_t)1 << 61) - digest_prefix))
        throw std::invalid_argument("digest_prefix must be a multiple of 64 with digest_prefix + the message length below 2^61");
}
// Selective disclosure, behind everything else a key emits: ceil(L / 8) mask bytes and L revealed bytes as inputs, the mask first (trace_layout.h TRV_*); one
// row mask_i * 1 = 0 per mask bit at or beyond L; per message bit ONE row mask_i * m_ij = r_ij with the mask input in A, the message witness of alloc_message_and_key
// in B and the revealed input in C.  No witness is allocated.  `bytes` = the trace length ahead of the region; returns the length with it
size_t reveal(Builder &b, const std::vector<Byte> &msg, size_t bytes) {
    const size_t len = msg.size(), mb = TRV_MASK_BYTES(len);
    const uint32_t rv = (uint32_t)TRV(bytes), rev = rv + (uint32_t)TRV_REVEALED(len);
    std::vector<Byte> mask(mb);
    for (size_t i = 0; i < mb; i++) mask[i] = b.alloc_byte(true, rv + TRV_MASK + (uint32_t)i);
    for (size_t i = len; i < 8 * mb; i++) b.enforce_equal(mask[i / 8][i % 8], Bit::konst(false));
    for (size_t i = 0; i < len; i++) {
        Byte r = b.alloc_byte(true, rev + (uint32_t)i);
        for (int k = 0; k < 8; k++) {
            LC A_, B_, C_;
            A_.add(1, mask[i / 8][i % 8]); B_.add(1, msg[i][k]); C_.add(1, r[k]);
            b.enforce(A_, B_, C_);
        }
    }
    return TRV_BYTES(bytes, 1, len);
}
void require_reveal(int reveal) {
    if (reveal != 0 && reveal != 1) throw std::invalid_argument("reveal must be 0 or 1");
}
// finish() for a mode whose own trace takes mode_bytes: the key-tag blocks go behind it, the digest region behind them, the reveal region last
Circuit finish_aes(Builder &b, AesGates &g, int kind, size_t n_blocks, size_t mode_bytes, size_t key_tag_blocks, const std::vector<Byte> &msg, int digest_kind, uint64_t digest_prefix, int rv) {
    size_t trace_bytes = g.key_tag(key_tag_blocks, mode_bytes);
    const size_t digest_off = digest_kind ? TRD(trace_bytes) : 0;
    if (digest_kind) { Sha256Gates sha(b); trace_bytes = sha.digest(msg, digest_kind, digest_prefix, trace_bytes); }
    const size_t reveal_off = rv ? TRV(trace_bytes) : 0;
    if (rv) trace_bytes = reveal(b, msg, trace_bytes);
    Circuit c = finish(b, kind, n_blocks, trace_bytes, g.key_bytes());
    c.key_tag_blocks = key_tag_blocks; c.key_tag_off = key_tag_blocks ? TRK_KT(mode_bytes) : 0;
    c.digest_kind = digest_kind; c.digest_prefix = digest_prefix; c.digest_blocks = TRD_BLOCKS(digest_kind, msg.size()); c.digest_off = digest_off;
    c.reveal = rv; c.reveal_off = reveal_off;
    return c;
}
}  // namespace

Circuit compile_aes_circuit(size_t len, size_t key_bits, size_t key_tag_blocks, int digest_kind, uint64_t digest_prefix, int reveal) {
    if (len % 16) throw std::invalid_argument("Input must be 16 bytes length when adding round key");
    require_key_bits(key_bits);
    require_key_tag_blocks(key_tag_blocks);
    require_digest(digest_kind, digest_prefix, len);
    require_reveal(reveal);
    size_t nb = len / 16;
    Builder b;
    AesGates g(b, key_bits);
    std::vector<Byte> msg = g.alloc_message_and_key(len);
    g.key_schedule();
    std::vector<Byte> ct(len);
    for (size_t bi = 0; bi < nb; bi++) {
        std::array<Byte, 16> s = g.block_rounds(&msg[16 * bi], bi);
        for (int i = 0; i < 16; i++) ct[16 * bi + i] = s[i];
    }
    g.ciphertext_inputs(ct);
    return finish_aes(b, g, CIRCUIT_AES, nb, TRK_ECB_BYTES(g.nk, nb), key_tag_blocks, msg, digest_kind, digest_prefix, reveal);
}

// Gate order: message and key witnesses, the 16 IV bytes as inputs, the key schedule, per block the 128 xor gates of X_b = M_b ^ prev (prev = the IV bytes, then the
// previous block's S_10) and the block's rounds from X_b, the ciphertext inputs.  The instance is One, 128 IV bits, 128 nb ciphertext bits.
Circuit compile_aes_cbc_circuit(size_t len, size_t key_bits, size_t key_tag_blocks, int digest_kind, uint64_t digest_prefix, int reveal) {
    if (len == 0 || len % 16) throw std::invalid_argument("CBC: the message must be a non-zero multiple of 16 bytes");
    require_key_bits(key_bits);
    require_key_tag_blocks(key_tag_blocks);
    require_digest(digest_kind, digest_prefix, len);
    require_reveal(reveal);
    size_t nb = len / 16;
    Builder b;
    AesGates g(b, key_bits);
    const uint32_t cbc = (uint32_t)TRK_CBC(g.nk, nb);
    std::vector<Byte> msg = g.alloc_message_and_key(len);
    std::array<Byte, 16> prev;
    for (int i = 0; i < 16; i++) prev[i] = b.alloc_byte(true, cbc + TR_CBC_IV + (uint32_t)i);
    g.key_schedule();
    std::vector<Byte> ct(len);
    for (size_t bi = 0; bi < nb; bi++) {
        std::array<Byte, 16> x;
        for (int i = 0; i < 16; i++) x[i] = b.xor_byte(msg[16 * bi + i], prev[i], cbc + TR_CBC_X + (uint32_t)(16 * bi + i));
        prev = g.block_rounds(x.data(), bi);
        for (int i = 0; i < 16; i++) ct[16 * bi + i] = prev[i];
    }
    g.ciphertext_inputs(ct);
    return finish_aes(b, g, CIRCUIT_AES_CBC, nb, cbc + TR_CBC_X + 16 * nb, key_tag_blocks, msg, digest_kind, digest_prefix, reveal);
}

// Gate order: message and key witnesses, the 16 ICB bytes as inputs, the key schedule, per block (from the second on) the incrementer over the previous block's counter
// bits, the block's rounds from CTR_b (so S_0 = CTR_b ^ key) and one xor gate per existing message bit, C = M ^ S_10; last the ciphertext inputs.  The instance is One,
// 128 ICB bits, 8 len ciphertext bits.
// Incrementer: counter bit i (weight 2^i) is bit i % 8 of byte 15 - i / 8.  c_0 = 1, y_i = x_i ^ c_i, c_{i+1} = x_i & c_i (none behind i = 127: the sum is mod 2^128).
// Position 0 folds away (y_0 = !x_0, c_1 = x_0), which leaves 127 xor and 126 and gates per increment.
Circuit compile_aes_ctr_circuit(size_t len, size_t key_bits, size_t key_tag_blocks, int digest_kind, uint64_t digest_prefix, int reveal) {
    if (len == 0) throw std::invalid_argument("CTR: the message must have at least one byte");
    require_key_bits(key_bits);
    require_key_tag_blocks(key_tag_blocks);
    require_digest(digest_kind, digest_prefix, len);
    require_reveal(reveal);
    size_t nb = (len + 15) / 16;
    Builder b;
    AesGates g(b, key_bits);
    const uint32_t ctr = (uint32_t)TRK_CTR(g.nk, nb);
    auto slot = [&](size_t bi) { return ctr + (uint32_t)(TR_CTR_BLOCK0 + bi * TR_CTR_BLOCK_STRIDE); };
    std::vector<Byte> msg = g.alloc_message_and_key(len);
    std::array<Byte, 16> cnt;
    for (int i = 0; i < 16; i++) cnt[i] = b.alloc_byte(true, ctr + TR_CTR_ICB + (uint32_t)i);
    g.key_schedule();
    std::vector<Byte> ct(len);
    for (size_t bi = 0; bi < nb; bi++) {
        if (bi) {
            std::array<Byte, 16> next;
            Bit carry = Bit::konst(true);
            for (int i = 0; i < 128; i++) {
                uint32_t byte = (uint32_t)(15 - i / 8);
                Bit x = cnt[byte][i % 8];
                uint32_t mark = b.n_witness;
                next[byte][i % 8] = b.bxor(x, carry);
                b.tag_bytebit(next[byte][i % 8], mark, slot(bi) + TR_CTR_BL_CTR + byte, i % 8);
                if (i == 127) break;
                mark = b.n_witness;
                carry = b.band(x, carry);
                b.tag_bytebit(carry, mark, slot(bi) + TR_CTR_BL_CARRY + byte, i % 8);
            }
            cnt = next;
        }
        std::array<Byte, 16> s = g.block_rounds(cnt.data(), bi);
        for (size_t i = 0; i < 16 && 16 * bi + i < len; i++) ct[16 * bi + i] = b.xor_byte(msg[16 * bi + i], s[i], slot(bi) + TR_CTR_BL_CT + (uint32_t)i);
    }
    for (size_t i = 0; i < len; i++) {
        Byte pi = b.alloc_byte(true, slot(i / 16) + TR_CTR_BL_CT + (uint32_t)(i % 16));
        for (int k = 0; k < 8; k++) b.enforce_equal(pi[k], ct[i][k]);
    }
    Circuit c = finish_aes(b, g, CIRCUIT_AES_CTR, nb, TRK_CTR_BYTES(g.nk, nb), key_tag_blocks, msg, digest_kind, digest_prefix, reveal);
    c.message_bytes = len;
    return c;
}

// Gate order: message and key witnesses, the 12 iv bytes and the aad as inputs, the key schedule, the rounds of the H block (slot nb, round-0 input the constant zero
// block) and of the J_0 block (slot nb + 1, iv || 00000001), per message block the rounds from iv || be32(b + 2) (the low 32 counter bits are constants: no incrementer),
// one xor gate per existing message bit, GHASH, the 128 xor gates of the tag, last the ciphertext and the tag inputs.  The instance is One, 96 iv bits, 8 alen aad bits,
// 8 len ciphertext bits, 128 tag bits.
// GHASH (SP 800-38D 6.3, 6.4).  Bit k of a block, k = 0 the coefficient of alpha^0, is bit 7 - k % 8 of byte k / 8.  V_0 = H, V_{i+1} = V_i alpha: new[0] = old[127],
// new[k] = old[k-1] ^ old[127] for k = 1, 2, 7, new[k] = old[k-1] otherwise (3 xor gates a step, 381 for the table, once per proof).  One multiplication Y = X H:
// p_{i,k} = x_i & V_i[k] (16,384 and gates), then per output bit k a boolean y_k, seven booleans q_{k,0..6} and ONE row (sum_i p_{i,k} - y_k - 2 sum_j 2^j q_{k,j}) * One = 0:
// y_k is the parity of the 128 products and q_k <= 64 their half.  The difference sits in A, as in enforce_equal, so A's row is 0 on a satisfied witness.  X_1 is the
// first block itself; X_m = Y_{m-1} ^ block m costs one xor gate per existing bit (zero padding and the constant length block cost none).
namespace {
// what the lone GCM compiler and the segment compiler share of GHASH.  Bit k of a block is bit 7 - k % 8 of byte k / 8
using Blk = std::array<Bit, 128>;
Blk to_blk(const Byte *bytes) { Blk r; for (int k = 0; k < 128; k++) r[k] = bytes[k / 8][7 - k % 8]; return r; }
// the V table of H at trace offset v_off: 3 xor gates a step
std::vector<Blk> ghash_v_table(Builder &b, const std::array<Byte, 16> &h_bytes, uint32_t v_off) {
    std::vector<Blk> V(128);
    V[0] = to_blk(h_bytes.data());
    for (int i = 1; i < 128; i++) {
        const Blk &o = V[i - 1];
        V[i][0] = o[127];
        for (int k = 1; k < 128; k++) {
            if (k == 1 || k == 2 || k == 7) { uint32_t mark = b.n_witness; V[i][k] = b.bxor(o[k - 1], o[127]); b.tag_bytebit(V[i][k], mark, v_off + (uint32_t)i, 7 - k); }   // (byte 0 of V_i)
            else V[i][k] = o[k - 1];
        }
    }
    return V;
}
// X = prev ^ blk, one xor gate per non-constant bit pair, tagged as the X of the multiplication at trace offset mul
Blk ghash_chain_xor(Builder &b, const Blk &prev, const Blk &blk, uint32_t mul) {
    Blk X;
    for (int k = 0; k < 128; k++) { uint32_t mark = b.n_witness; X[k] = b.bxor(prev[k], blk[k]); b.tag_bytebit(X[k], mark, mul + TR_GCM_MUL_X + (uint32_t)(k / 8), 7 - k % 8); }
    return X;
}
// Y = X H: the products, then per output bit y, seven q and the parity row
Blk ghash_multiply(Builder &b, const Blk &X, const std::vector<Blk> &V, uint32_t mul) {
    std::vector<Bit> p(128 * 128);
    Blk Y;
    for (int i = 0; i < 128; i++) for (int k = 0; k < 128; k++) {
        uint32_t mark = b.n_witness;
        p[128 * i + k] = b.band(X[i], V[i][k]);
        b.tag_bytebit(p[128 * i + k], mark, mul + TR_GCM_MUL_P + (uint32_t)(128 * (k / 8) + i), 7 - k % 8);
    }
    for (int k = 0; k < 128; k++) {
        Y[k] = b.alloc(false, mul + TR_GCM_MUL_Y + (uint32_t)(k / 8), 7 - k % 8);
        LC d, one, z;
        for (int i = 0; i < 128; i++) d.add(1, p[128 * i + k]);
        d.add(-1, Y[k]);
        for (int j = 0; j < 7; j++) d.add(-(int64_t)(2 << j), b.alloc(false, mul + TR_GCM_MUL_Q + (uint32_t)k, j));
        one.add(1, 0u);
        b.enforce(d, one, z);
    }
    return Y;
}
}  // namespace

Circuit compile_aes_gcm_circuit(size_t len, size_t alen, size_t key_bits, size_t key_tag_blocks, int digest_kind, uint64_t digest_prefix, int reveal) {
    require_key_bits(key_bits);
    require_key_tag_blocks(key_tag_blocks);
    require_digest(digest_kind, digest_prefix, len);
    require_reveal(reveal);
    if (len == 0) throw std::invalid_argument("GCM: the message must have at least one byte");
    if (len > (1u << 16) || alen > (1u << 16)) throw std::invalid_argument("GCM: message and aad of one proof are limited to 65536 bytes each");
    const size_t nb = (len + 15) / 16, na = (alen + 15) / 16, n_mul = TR_GCM_MULS(na, nb);
    const uint32_t gcm = (uint32_t)TRK_GCM(key_bits / 32, nb);
    Builder b;
    AesGates g(b, key_bits);
    std::vector<Byte> msg = g.alloc_message_and_key(len);
    std::array<Byte, 16> in;
    for (int i = 0; i < 12; i++) in[i] = b.alloc_byte(true, gcm + TR_GCM_IV + (uint32_t)i);
    std::vector<Byte> aad(16 * na, Builder::const_byte(0)), ct(16 * nb, Builder::const_byte(0));
    for (size_t i = 0; i < alen; i++) aad[i] = b.alloc_byte(true, gcm + TR_GCM_AAD + (uint32_t)i);
    g.key_schedule();
    std::array<Byte, 16> zero;
    for (int i = 0; i < 16; i++) zero[i] = Builder::const_byte(0);
    const std::array<Byte, 16> h_bytes = g.block_rounds(zero.data(), nb);
    auto counter = [&](uint32_t n) { for (int i = 0; i < 4; i++) in[12 + i] = Builder::const_byte((uint8_t)(n >> (24 - 8 * i))); return in.data(); };
    const std::array<Byte, 16> ej0 = g.block_rounds(counter(1), nb + 1);
    std::vector<std::array<Byte, 16>> ks(nb);
    for (size_t bi = 0; bi < nb; bi++) ks[bi] = g.block_rounds(counter((uint32_t)bi + 2), bi);
    for (size_t i = 0; i < len; i++) ct[i] = b.xor_byte(msg[i], ks[i / 16][i % 16], gcm + (uint32_t)(TR_GCM_CT(na) + i));
    // ---- GHASH: the V table
    const std::vector<Blk> V = ghash_v_table(b, h_bytes, gcm + (uint32_t)TR_GCM_V(na, nb));
    // ---- the blocks GHASH runs over: the aad, the ciphertext (the bits of the C = M ^ S_10 gates), the length block
    std::vector<Blk> blocks;
    for (size_t j = 0; j < na; j++) blocks.push_back(to_blk(&aad[16 * j]));
    for (size_t j = 0; j < nb; j++) blocks.push_back(to_blk(&ct[16 * j]));
    {
        std::array<Byte, 16> lb;
        for (int i = 0; i < 8; i++) { lb[i] = Builder::const_byte((uint8_t)((uint64_t)(8 * alen) >> (56 - 8 * i))); lb[8 + i] = Builder::const_byte((uint8_t)((uint64_t)(8 * len) >> (56 - 8 * i))); }
        blocks.push_back(to_blk(lb.data()));
    }
    Blk X = blocks[0], Y;
    for (size_t m = 0; m < n_mul; m++) {
        const uint32_t mul = gcm + (uint32_t)(TR_GCM_MUL0(na, nb) + m * TR_GCM_MUL_STRIDE);
        if (m) X = ghash_chain_xor(b, Y, blocks[m], mul);
        Y = ghash_multiply(b, X, V, mul);
    }
    // ---- tag = S ^ AES_K(J_0), then the public ciphertext and tag
    const uint32_t tag_off = gcm + (uint32_t)TR_GCM_TAG(na, nb);
    std::array<Byte, 16> tag;
    for (int j = 0; j < 16; j++) { Byte s; for (int bit = 0; bit < 8; bit++) s[bit] = Y[8 * j + 7 - bit]; tag[j] = b.xor_byte(s, ej0[j], tag_off + (uint32_t)j); }
    for (size_t i = 0; i < len; i++) {
        Byte pi = b.alloc_byte(true, gcm + (uint32_t)(TR_GCM_CT(na) + i));
        for (int k = 0; k < 8; k++) b.enforce_equal(pi[k], ct[i][k]);
    }
    for (int j = 0; j < 16; j++) {
        Byte pi = b.alloc_byte(true, tag_off + (uint32_t)j);
        for (int k = 0; k < 8; k++) b.enforce_equal(pi[k], tag[j][k]);
    }
    Circuit c = finish_aes(b, g, CIRCUIT_AES_GCM, nb, TRK_GCM_BYTES(g.nk, na, nb), key_tag_blocks, msg, digest_kind, digest_prefix, reveal);
    c.message_bytes = len; c.aad_bytes = alen;
    return c;
}

// One segment of a GCM record.  Gate order: message and key witnesses; the 12 iv bytes, the 4 ctr0 bytes and (head) the aad as inputs; the Y_in, salt_in
// (mid, tail) and salt_out (head, mid) witnesses; the key schedule; the rounds of the H block (slot nb) and, for a tail, of the J_0 block (slot nb + 1); per data block
// from the second on the incrementer over the previous block's low 32 counter bits (position 0 folds away as in CTR: 31 xor and 30 and gates, no carry out of
// position 31) and the block's rounds from iv || counter; one xor gate per existing message bit; the ciphertext inputs and (tail) the 128 length-block inputs; the V
// table; GHASH -- a head starts at its first block as the lone circuit does, a mid or tail with X_0 = Y_in ^ C_0, and a tail's last multiplication runs over the
// length-block INPUTS; (tail) the tag's xor gates and inputs; last com_in (mid, tail), then com_out (head, mid): 256 inputs each, one compression from the constant
// initial value over key || zeros || Y || salt, 256 equalities.  A head with key_tag_blocks = T then has the T tag blocks of key_tag() and their 128 T
// inputs.  With reveal = 1 the mask and revealed inputs and their rows (reveal() above) come last of all.
// With digest = 1 a head or mid ends in 9f's chain digest over its 16 c bytes, the new role "last" (a mid of `units` = Lr BYTES, the final block cut and
// zero-padded for GHASH as a tail's) in a final digest whose length field is the eight total_bits INPUTS, and the tail is the data-less closing tail: units = 0, no
// message, the H slot and the J_0 slot, ONE multiplication over X = Y_in ^ the length block, the tag, com_in.  The digest region's inputs -- H_in, H_out, (last)
// total_bits -- come last of all.
Circuit compile_aes_gcm_segment_circuit(int role, size_t units, size_t alen, size_t key_bits, int rv, size_t key_tag_blocks, int digest) {
    require_key_bits(key_bits);
    require_reveal(rv);
    require_key_tag_blocks(key_tag_blocks);
    if (digest != 0 && digest != 1) throw std::invalid_argument("GCM segment: digest must be 0 or 1");
    if (!digest) {
        if (role != TRS_HEAD && role != TRS_MID && role != TRS_TAIL)
            throw std::invalid_argument("GCM segment: the role must be 0 (head), 1 (mid) or 2 (tail); 3 (last) belongs to a digest record: use the _gcm_seg_dg entries (zkaes_synthesize_keys_gcm_seg_dg)");
    } else {
        if (role != TRS_HEAD && role != TRS_MID && role != TRS_TAIL && role != TRS_LAST) throw std::invalid_argument("GCM digest segment: the role must be 0 (head), 1 (mid), 2 (tail) or 3 (last)");
        if (rv) throw std::invalid_argument("GCM digest segment: a digest segment key has no reveal form: use a reveal segment key without a digest (zkaes_synthesize_keys_gcm_seg_rv), or a lone GCM key with digest and reveal for a record of one proof");
        if (key_tag_blocks) throw std::invalid_argument("GCM digest segment: a digest segment key takes no key_tag_blocks (a tagged digest head does not fit the default SRS): use a tagged head without a digest (zkaes_synthesize_keys_gcm_seg_kt)");
        if ((role == TRS_HEAD || role == TRS_MID) && (16 * units) % 64)
            throw std::invalid_argument("GCM digest segment: SHA-256 absorbs 64 bytes at a time, so a digest head or mid holds whole 64-byte blocks: use c, the data blocks per segment, a multiple of 4");
        if (role == TRS_TAIL && units) throw std::invalid_argument("GCM digest segment: the tail of a digest record holds no data: use units = 0 for it, and role 3 (last) with units = the last data bytes for the segment ahead of it");
    }
    if (role != TRS_HEAD && key_tag_blocks)
        throw std::invalid_argument("GCM segment: only the head segment takes key_tag_blocks: the head carries the record's key tag and the boundary commitments carry the key to every later segment");
    const bool begins = role == TRS_HEAD, ends = role == TRS_TAIL, bytes_role = ends || role == TRS_LAST;
    if (units == 0 && !(digest && ends))
        throw std::invalid_argument("GCM segment: a head or mid has at least one data block, a tail at least one byte (a tail of 0 bytes is the closing tail of a digest record: the _gcm_seg_dg entries)");
    if (role != TRS_HEAD && alen) throw std::invalid_argument("GCM segment: only the head segment takes the aad");
    if (units > (1u << 16) || alen > (1u << 16)) throw std::invalid_argument("GCM segment: message and aad of one proof are limited to 65536 bytes each");
    const size_t len = bytes_role ? units : 16 * units, nb = (len + 15) / 16, na = (alen + 15) / 16, n_mul = TRS_MULS(role, na, nb);
    const int nk = (int)(key_bits / 32);
    const uint32_t gcm = (uint32_t)TRS_GCM(nk, role, nb), sg = gcm + (uint32_t)TRS_SEG(role, na, nb);
    Builder b;
    AesGates g(b, key_bits);
    std::vector<Byte> msg = g.alloc_message_and_key(len);
    std::array<Byte, 16> in, yin, salt_in, salt_out;
    for (int i = 0; i < 16; i++) in[i] = b.alloc_byte(true, gcm + TR_GCM_IV + (uint32_t)i);          // iv, then ctr0
    std::vector<Byte> aad(16 * na, Builder::const_byte(0)), ct(16 * nb, Builder::const_byte(0));
    for (size_t i = 0; i < alen; i++) aad[i] = b.alloc_byte(true, gcm + TR_GCM_AAD + (uint32_t)i);
    if (!begins) for (int i = 0; i < 16; i++) yin[i] = b.alloc_byte(false, sg + TRS_YIN + (uint32_t)i);
    if (!begins) for (int i = 0; i < 16; i++) salt_in[i] = b.alloc_byte(false, sg + TRS_SALT_IN + (uint32_t)i);
    if (!ends) for (int i = 0; i < 16; i++) salt_out[i] = b.alloc_byte(false, sg + TRS_SALT_OUT + (uint32_t)i);
    g.key_schedule();
    std::array<Byte, 16> zero, j0 = in;
    for (int i = 0; i < 16; i++) zero[i] = Builder::const_byte(0);
    const std::array<Byte, 16> h_bytes = g.block_rounds(zero.data(), nb);
    std::array<Byte, 16> ej0;
    if (ends) {
        for (int i = 0; i < 4; i++) j0[12 + i] = Builder::const_byte(i == 3 ? 1 : 0);
        ej0 = g.block_rounds(j0.data(), nb + 1);
    }
    for (size_t bi = 0; bi < nb; bi++) {
        if (bi) {
            const uint32_t slot = sg + (uint32_t)(TRS_BLOCK_CTR0 + bi * TRS_BLOCK_CTR_STRIDE);
            std::array<Byte, 16> next = in;
            Bit carry = Bit::konst(true);
            for (int i = 0; i < 32; i++) {
                const uint32_t byte = (uint32_t)(3 - i / 8);
                Bit x = in[12 + byte][i % 8];
                uint32_t mark = b.n_witness;
                next[12 + byte][i % 8] = b.bxor(x, carry);
                b.tag_bytebit(next[12 + byte][i % 8], mark, slot + TRS_BL_CTR + byte, i % 8);
                if (i == 31) break;
                mark = b.n_witness;
                carry = b.band(x, carry);
                b.tag_bytebit(carry, mark, slot + TRS_BL_CARRY + byte, i % 8);
            }
            in = next;
        }
        const std::array<Byte, 16> ks = g.block_rounds(in.data(), bi);
        for (size_t i = 0; i < 16 && 16 * bi + i < len; i++) ct[16 * bi + i] = b.xor_byte(msg[16 * bi + i], ks[i], gcm + (uint32_t)(TR_GCM_CT(na) + 16 * bi + i));
    }
    for (size_t i = 0; i < len; i++) {
        Byte pi = b.alloc_byte(true, gcm + (uint32_t)(TR_GCM_CT(na) + i));
        for (int k = 0; k < 8; k++) b.enforce_equal(pi[k], ct[i][k]);
    }
    std::array<Byte, 16> lb;
    if (ends) for (int i = 0; i < 16; i++) lb[i] = b.alloc_byte(true, sg + TRS_LEN + (uint32_t)i);
    // ---- GHASH
    const std::vector<Blk> V = ghash_v_table(b, h_bytes, gcm + (uint32_t)TR_GCM_V(na, nb));
    std::vector<Blk> blocks;
    for (size_t j = 0; j < na; j++) blocks.push_back(to_blk(&aad[16 * j]));
    for (size_t j = 0; j < nb; j++) blocks.push_back(to_blk(&ct[16 * j]));
    if (ends) blocks.push_back(to_blk(lb.data()));
    Blk X, Y;
    if (!begins) Y = to_blk(yin.data());
    for (size_t m = 0; m < n_mul; m++) {
        const uint32_t mul = gcm + (uint32_t)(TR_GCM_MUL0(na, nb) + m * TR_GCM_MUL_STRIDE);
        if (m || !begins) X = ghash_chain_xor(b, Y, blocks[m], mul); else X = blocks[0];
        Y = ghash_multiply(b, X, V, mul);
    }
    if (ends) {
        const uint32_t tag_off = gcm + (uint32_t)TRS_TAG(role, na, nb);
        std::array<Byte, 16> tag;
        for (int j = 0; j < 16; j++) { Byte s; for (int bit = 0; bit < 8; bit++) s[bit] = Y[8 * j + 7 - bit]; tag[j] = b.xor_byte(s, ej0[j], tag_off + (uint32_t)j); }
        for (int j = 0; j < 16; j++) {
            Byte pi = b.alloc_byte(true, tag_off + (uint32_t)j);
            for (int k = 0; k < 8; k++) b.enforce_equal(pi[k], tag[j][k]);
        }
    }
    // ---- the boundary commitments
    Sha256Gates sha(b);
    auto commit = [&](const std::array<Byte, 16> &y, const std::array<Byte, 16> &salt, uint32_t com_off, uint32_t slot) {
        std::array<Byte, 64> blk;
        for (size_t i = 0; i < 32; i++) blk[i] = i < g.key_bytes() ? g.key[i] : Builder::const_byte(0);
        for (int i = 0; i < 16; i++) { blk[32 + i] = y[i]; blk[48 + i] = salt[i]; }
        std::array<Byte, 32> pi;
        for (int j = 0; j < 32; j++) pi[j] = b.alloc_byte(true, com_off + (uint32_t)j);
        std::array<Word, 8> st;
        for (int k = 0; k < 8; k++) st[k] = Sha256Gates::const_word(SHA256_IV[k]);
        std::array<Word, 16> words;
        for (int t = 0; t < 16; t++) words[t] = Sha256Gates::be_word(&blk[4 * t]);
        st = sha.compress(st, words, slot);
        for (int j = 0; j < 32; j++) for (int k = 0; k < 8; k++) b.enforce_equal(pi[j][k], st[j / 4][8 * (3 - j % 4) + k]);
    };
    if (!begins) commit(yin, salt_in, sg + TRS_COM_IN, sg + (uint32_t)TRS_SLOT_IN(nb));
    if (!ends) {
        std::array<Byte, 16> yout;
        for (int j = 0; j < 16; j++) for (int bit = 0; bit < 8; bit++) yout[j][bit] = Y[8 * j + 7 - bit];
        commit(yout, salt_out, sg + TRS_COM_OUT, sg + (uint32_t)TRS_SLOT_OUT(nb));
    }
    // ---- the key tag of a head: the tag slots behind the segment region and its compression slots, as finish_aes puts them behind a mode's tail
    const size_t seg_bytes = TRS_BYTES(nk, role, na, nb);
    size_t trace_bytes = g.key_tag(key_tag_blocks, seg_bytes);
    // ---- selective disclosure: the segment's slice of the record's mask and revealed bytes, behind the commitments as finish_aes puts them behind the digest
    // ---- the digest of a digest record's data segment: 9f's region behind the segment region and its compression slots, as finish_aes puts it behind a
    // mode's tail (a digest key has neither tag blocks nor reveal, so nothing lies between or behind)
    const int digest_kind = digest ? TRS_DG_KIND(role) : DIGEST_NONE;
    const size_t digest_off = digest_kind ? TRD(trace_bytes) : 0;
    if (digest_kind) trace_bytes = sha.digest(msg, digest_kind, 0, trace_bytes, role == TRS_LAST);
    const size_t reveal_off = rv ? TRV(trace_bytes) : 0;
    if (rv) trace_bytes = reveal(b, msg, trace_bytes);
    Circuit c = finish(b, CIRCUIT_AES_GCM_SEG, nb, trace_bytes, g.key_bytes());
    c.message_bytes = len; c.aad_bytes = alen; c.seg_role = role; c.seg_off = sg; c.seg_digest = digest;
    c.digest_kind = digest_kind; c.digest_blocks = TRD_BLOCKS(digest_kind, len); c.digest_off = digest_off;
    c.key_tag_blocks = key_tag_blocks; c.key_tag_off = key_tag_blocks ? TRK_KT(seg_bytes) : 0;
    c.reveal = rv; c.reveal_off = reveal_off;
    return c;
}

Circuit compile_circuit(int kind, size_t message_len, size_t aad_len, size_t key_bits, size_t key_tag_blocks, int digest_kind, uint64_t digest_prefix, int reveal) {
    require_reveal(reveal);
    if (kind == CIRCUIT_AES_GCM_SEG) throw std::invalid_argument("a GCM segment circuit has a role: use the _gcm_seg entry points (zkaes_circuit_info_gcm_seg, zkaes_synthesize_keys_gcm_seg); through the plain queries segments have no reveal form, their _gcm_seg_rv entries take the flag");
    if (kind == CIRCUIT_AES_GCM)return compile_aes_gcm_circuit(message_len, aad_len, key_bits, key_tag_blocks, digest_kind, digest_prefix, reveal);
    if (aad_len) throw std::invalid_argument("only a GCM circuit takes additional authenticated data");
    if (kind == CIRCUIT_AES) return compile_aes_circuit(message_len, key_bits, key_tag_blocks, digest_kind, digest_prefix, reveal);
    if (kind == CIRCUIT_AES_CBC) return compile_aes_cbc_circuit(message_len, key_bits, key_tag_blocks, digest_kind, digest_prefix, reveal);
    if (kind == CIRCUIT_AES_CTR) return compile_aes_ctr_circuit(message_len, key_bits, key_tag_blocks, digest_kind, digest_prefix, reveal);
    if (digest_kind || digest_prefix) throw std::invalid_argument("the ops circuits have no message: digest_kind must be 0");
    if (reveal) throw std::invalid_argument("the ops circuits have no message: reveal must be 0");
    if (key_bits != 128) throw std::invalid_argument("the ops circuits have no AES key: key_bits must be 128");
    if (key_tag_blocks) throw std::invalid_argument("the ops circuits have no AES key: key_tag_blocks must be 0");
    return compile_ops_circuit(kind);
}

namespace {
// plain byte-wise AES over aes_sbox_value for the host-side modes; key_len = 16, 24 or 32 bytes (the name dates from when 16 was the only one)
struct HostAes128 {
    uint8_t sb[256], rk[15][16];                                              // FIPS-197 5.2, round keys as 16 bytes in word order: rk[r] = W_4r .. W_4r+3
    int nr;
    static uint8_t xt(uint8_t c) { return (uint8_t)((c << 1) ^ ((c >> 7) * 0x1B)); }
    explicit HostAes128(const uint8_t *key, size_t key_len = 16) {
        if (key_len != 16 && key_len != 24 && key_len != 32) throw std::invalid_argument("the AES key must have 16, 24 or 32 bytes");
        const int nk = (int)(key_len / 4);
        nr = nk + 6;
        for (int i = 0; i < 256; i++) sb[i] = aes_sbox_value((uint8_t)i);
        uint8_t *w = &rk[0][0];                                               // word i at w + 4 i
        for (size_t i = 0; i < key_len; i++) w[i] = key[i];
        uint8_t rc = 1;
        for (int i = nk; i < 4 * (nr + 1); i++) {
            const uint8_t *p = w + 4 * (i - 1);
            uint8_t t[4] = {p[0], p[1], p[2], p[3]};
            if (i % nk == 0) { t[0] = (uint8_t)(sb[p[1]] ^ rc); t[1] = sb[p[2]]; t[2] = sb[p[3]]; t[3] = sb[p[0]]; rc = xt(rc); }
            else if (nk == 8 && i % 8 == 4) for (int k = 0; k < 4; k++) t[k] = sb[p[k]];
            for (int k = 0; k < 4; k++) w[4 * i + k] = (uint8_t)(w[4 * (i - nk) + k] ^ t[k]);
        }
    }
    void encrypt_block(uint8_t s[16]) const {                                 // in place
        uint8_t u[16];
        for (int i = 0; i < 16; i++) s[i] ^= rk[0][i];
        for (int r = 1; r <= nr; r++) {
            for (int c = 0; c < 4; c++) for (int rr = 0; rr < 4; rr++) u[4 * c + rr] = sb[s[4 * ((c + rr) & 3) + rr]];     // SubBytes + ShiftRows
            for (int c = 0; c < 4; c++) {
                const uint8_t *a = u + 4 * c;
                for (int k = 0; k < 4; k++)
                    s[4 * c + k] = (uint8_t)((r < nr ? xt(a[k]) ^ xt(a[(k + 1) & 3]) ^ a[(k + 1) & 3] ^ a[(k + 2) & 3] ^ a[(k + 3) & 3] : a[k]) ^ rk[r][4 * c + k]);
            }
        }
    }
};
}  // namespace

void aes_ecb_encrypt_host(const uint8_t *msg, size_t len, const uint8_t *key, size_t key_len, uint8_t *out) {
    if (len % 16) throw std::invalid_argument("ECB: the message must be a multiple of 16 bytes");
    HostAes128 aes(key, key_len);
    uint8_t s[16];
    for (size_t off = 0; off < len; off += 16) {
        for (int i = 0; i < 16; i++) s[i] = msg[off + i];
        aes.encrypt_block(s);
        for (int i = 0; i < 16; i++) out[off + i] = s[i];
    }
}

void aes_key_tag_block(size_t t, uint8_t out[16]) {
    static const char prefix[] = TRK_KT_D_PREFIX;
    for (int i = 0; i < 11; i++) out[i] = (uint8_t)prefix[i];
    out[11] = (uint8_t)t;
    for (int i = 12; i < 16; i++) out[i] = 0;
}

void aes_key_tag_host(const uint8_t *key, size_t key_len, size_t tag_blocks, uint8_t *out) {
    if (tag_blocks != 1 && tag_blocks != 2) throw std::invalid_argument("a key tag has 1 or 2 blocks");
    HostAes128 aes(key, key_len);
    for (size_t t = 0; t < tag_blocks; t++) { aes_key_tag_block(t, out + 16 * t); aes.encrypt_block(out + 16 * t); }
}

void aes128_cbc_encrypt_host(const uint8_t *msg, size_t len, const uint8_t *key, const uint8_t iv[16], uint8_t *out, size_t key_len) {
    if (len % 16) throw std::invalid_argument("CBC: the message must be a multiple of 16 bytes");
    HostAes128 aes(key, key_len);
    uint8_t prev[16], s[16];
    for (int i = 0; i < 16; i++) prev[i] = iv[i];
    for (size_t off = 0; off < len; off += 16) {
        for (int i = 0; i < 16; i++) s[i] = (uint8_t)(msg[off + i] ^ prev[i]);
        aes.encrypt_block(s);
        for (int i = 0; i < 16; i++) out[off + i] = prev[i] = s[i];
    }
}

void ctr_counter_add(const uint8_t counter[16], uint64_t n, uint8_t out[16]) {
    unsigned carry = 0;
    for (int i = 15; i >= 0; i--) {
        unsigned t = counter[i] + (unsigned)(n & 0xff) + carry;
        out[i] = (uint8_t)t; carry = t >> 8; n >>= 8;
    }
}

void aes128_ctr_crypt_host(const uint8_t *in, size_t len, const uint8_t *key, const uint8_t icb[16], uint8_t *out, size_t key_len) {
    HostAes128 aes(key, key_len);
    uint8_t ctr[16], s[16];
    for (int i = 0; i < 16; i++) ctr[i] = icb[i];
    for (size_t off = 0; off < len; off += 16) {
        for (int i = 0; i < 16; i++) s[i] = ctr[i];
        aes.encrypt_block(s);
        for (size_t i = 0; i < 16 && off + i < len; i++) out[off + i] = (uint8_t)(in[off + i] ^ s[i]);
        ctr_counter_add(ctr, 1, ctr);
    }
}

namespace {
// a GF(2^128) element in GCM's convention as two words: bit k (the coefficient of alpha^k) is bit 63 - k of hi for k < 64, bit 127 - k of lo behind
struct Gf128 { uint64_t hi = 0, lo = 0; };
Gf128 gf_load(const uint8_t b[16]) { Gf128 r; for (int i = 0; i < 8; i++) { r.hi = (r.hi << 8) | b[i]; r.lo = (r.lo << 8) | b[8 + i]; } return r; }
// SP 800-38D Algorithm 1: Z = X * Y, one conditional xor and one multiplication of V by alpha per bit of X
Gf128 gf_mul(const Gf128 &x, const Gf128 &y) {
    Gf128 z, v = y;
    for (int i = 0; i < 128; i++) {
        uint64_t xi = i < 64 ? (x.hi >> (63 - i)) & 1 : (x.lo >> (127 - i)) & 1;
        if (xi) { z.hi ^= v.hi; z.lo ^= v.lo; }
        uint64_t lsb = v.lo & 1;
        v.lo = (v.lo >> 1) | (v.hi << 63); v.hi >>= 1;
        if (lsb) v.hi ^= 0xE100000000000000ull;                                    // R = 11100001 || 0^120
    }
    return z;
}
}  // namespace

void aes128_gcm_encrypt_host(const uint8_t *msg, size_t len, const uint8_t *key, const uint8_t iv[12], const uint8_t *aad, size_t aad_len, uint8_t *ct, uint8_t tag[16], size_t key_len) {
    HostAes128 aes(key, key_len);
    uint8_t hb[16] = {0}, s[16], blk[16];
    aes.encrypt_block(hb);
    const Gf128 h = gf_load(hb);
    auto counter = [&](uint32_t n) { for (int i = 0; i < 12; i++) s[i] = iv[i]; for (int i = 0; i < 4; i++) s[12 + i] = (uint8_t)(n >> (24 - 8 * i)); aes.encrypt_block(s); };
    for (size_t off = 0; off < len; off += 16) {
        counter((uint32_t)(off / 16 + 2));
        for (size_t i = 0; i < 16 && off + i < len; i++) ct[off + i] = (uint8_t)(msg[off + i] ^ s[i]);
    }
    Gf128 y;
    auto absorb = [&](const uint8_t *data, size_t n) {                             // zero-padded to whole blocks
        for (size_t off = 0; off < n; off += 16) {
            for (size_t i = 0; i < 16; i++) blk[i] = off + i < n ? data[off + i] : 0;
            Gf128 x = gf_load(blk);
            x.hi ^= y.hi; x.lo ^= y.lo;
            y = gf_mul(x, h);
        }
    };
    absorb(aad, aad_len);
    absorb(ct, len);
    Gf128 x;
    x.hi = y.hi ^ (uint64_t)aad_len * 8; x.lo = y.lo ^ (uint64_t)len * 8;
    y = gf_mul(x, h);
    counter(1);
    for (int i = 0; i < 8; i++) { tag[i] = (uint8_t)((y.hi >> (56 - 8 * i)) ^ s[i]); tag[8 + i] = (uint8_t)((y.lo >> (56 - 8 * i)) ^ s[8 + i]); }
}

void gcm_boundaries_host(const uint8_t *msg, size_t len, const uint8_t *key, size_t key_len, const uint8_t iv[12], const uint8_t *aad, size_t aad_len, size_t c, uint8_t *ys) {
    if (len == 0 || c == 0) throw std::invalid_argument("gcm_boundaries: the record must have at least one byte and a segment at least one block");
    std::vector<uint8_t> ct(len);
    uint8_t tag[16], hb[16] = {0}, blk[16];
    aes128_gcm_encrypt_host(msg, len, key, iv, aad, aad_len, ct.data(), tag, key_len);
    HostAes128 aes(key, key_len);
    aes.encrypt_block(hb);
    const Gf128 h = gf_load(hb);
    Gf128 y;
    for (size_t off = 0; off < aad_len; off += 16) {
        for (size_t i = 0; i < 16; i++) blk[i] = off + i < aad_len ? aad[off + i] : 0;
        Gf128 x = gf_load(blk);
        x.hi ^= y.hi; x.lo ^= y.lo;
        y = gf_mul(x, h);
    }
    const size_t nb = (len + 15) / 16, n = (nb + c - 1) / c;
    for (size_t bi = 0; bi < nb; bi++) {
        for (size_t i = 0; i < 16; i++) blk[i] = 16 * bi + i < len ? ct[16 * bi + i] : 0;
        Gf128 x = gf_load(blk);
        x.hi ^= y.hi; x.lo ^= y.lo;
        y = gf_mul(x, h);
        if ((bi + 1) % c == 0 && (bi + 1) / c < n)                                  // the last block of segment s = (bi + 1) / c - 1 < n - 1
            for (int i = 0; i < 8; i++) { ys[16 * ((bi + 1) / c - 1) + i] = (uint8_t)(y.hi >> (56 - 8 * i)); ys[16 * ((bi + 1) / c - 1) + 8 + i] = (uint8_t)(y.lo >> (56 - 8 * i)); }
    }
}

void gcm_commit_host(const uint8_t *key, size_t key_len, const uint8_t y[16], const uint8_t salt[16], uint8_t com[32]) {
    if (key_len != 16 && key_len != 24 && key_len != 32) throw std::invalid_argument("the AES key must have 16, 24 or 32 bytes");
    uint8_t blk[64] = {0};
    for (size_t i = 0; i < key_len; i++) blk[i] = key[i];
    for (int i = 0; i < 16; i++) { blk[32 + i] = y[i]; blk[48 + i] = salt[i]; }
    sha256_chain(nullptr, blk, 64, com);
}

// src/ops.rs:8-29.  Trace: x (4 B LE) | y (4 B LE) | result (8 B LE)
Circuit compile_ops_circuit(int kind) {
    Builder b;
    Word x, y;
    for (int i = 0; i < 32; i++) x[i] = b.alloc(false, (uint32_t)(i / 8), i % 8);
    for (int i = 0; i < 32; i++) y[i] = b.alloc(false, (uint32_t)(4 + i / 8), i % 8);
    if (kind == CIRCUIT_OPS_XOR) {
        for (int i = 0; i < 32; i++) { uint32_t mark = b.n_witness; Bit r = b.bxor(x[i], y[i]); b.tag_bytebit(r, mark, (uint32_t)(8 + i / 8), i % 8); }
    } else {
        // UInt32::addmany: 33 result bits (max_value = 2 * u32::MAX), then 0 * 0 = sum(2^i x_i) + sum(2^i y_i) - sum(2^i r_i)
        LC lc;
        int64_t coeff = 1;
        for (int i = 0; i < 32; i++) { lc.add(coeff, x[i]); coeff *= 2; }
        coeff = 1;
        for (int i = 0; i < 32; i++) { lc.add(coeff, y[i]); coeff *= 2; }
        coeff = 1;
        for (int i = 0; i < 33; i++) { Bit r = b.alloc(false, (uint32_t)(8 + i / 8), i % 8); lc.add(-coeff, r.var()); coeff *= 2; }
        LC z;
        b.enforce(z, z, lc);
    }
    return finish(b, kind, 0, 16);
}

namespace {
inline uint32_t rotr32(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
void sha256_compress(uint32_t st[8], const uint8_t blk[64]) {
    uint32_t w[64];
    for (int t = 0; t < 16; t++) w[t] = (uint32_t)blk[4 * t] << 24 | (uint32_t)blk[4 * t + 1] << 16 | (uint32_t)blk[4 * t + 2] << 8 | blk[4 * t + 3];
    for (int t = 16; t < 64; t++) {
        uint32_t s0 = rotr32(w[t - 15], 7) ^ rotr32(w[t - 15], 18) ^ (w[t - 15] >> 3), s1 = rotr32(w[t - 2], 17) ^ rotr32(w[t - 2], 19) ^ (w[t - 2] >> 10);
        w[t] = s1 + w[t - 7] + s0 + w[t - 16];
    }
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
    for (int t = 0; t < 64; t++) {
        uint32_t t1 = h + (rotr32(e, 6) ^ rotr32(e, 11) ^ rotr32(e, 25)) + ((e & f) ^ (~e & g)) + SHA256_K[t] + w[t];
        uint32_t t2 = (rotr32(a, 2) ^ rotr32(a, 13) ^ rotr32(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}
void sha256_load(uint32_t st[8], const uint8_t *h_in) {
    for (int k = 0; k < 8; k++) st[k] = h_in ? (uint32_t)h_in[4 * k] << 24 | (uint32_t)h_in[4 * k + 1] << 16 | (uint32_t)h_in[4 * k + 2] << 8 | h_in[4 * k + 3] : SHA256_IV[k];
}
void sha256_store(const uint32_t st[8], uint8_t out[32]) { for (int k = 0; k < 8; k++) for (int i = 0; i < 4; i++) out[4 * k + i] = (uint8_t)(st[k] >> (24 - 8 * i)); }
}  // namespace

void sha256_chain(const uint8_t *h_in, const uint8_t *data, size_t len, uint8_t h_out[32]) {
    if (len % 64) throw std::invalid_argument("sha256_chain: the data must be a multiple of 64 bytes");
    uint32_t st[8];
    sha256_load(st, h_in);
    for (size_t off = 0; off < len; off += 64) sha256_compress(st, data + off);
    sha256_store(st, h_out);
}

void sha256_finish(const uint8_t *h_in, uint64_t prefix_bytes, const uint8_t *tail, size_t tail_len, uint8_t digest[32]) {
    if (prefix_bytes % 64 || prefix_bytes >= ((uint64_t)1 << 61) || (uint64_t)tail_len >= ((uint64_t)1 << 61) - prefix_bytes)
        throw std::invalid_argument("sha256_finish: prefix_bytes must be a multiple of 64 with prefix_bytes + tail_len below 2^61");
    uint32_t st[8];
    sha256_load(st, h_in);
    size_t off = 0;
    for (; off + 64 <= tail_len; off += 64) sha256_compress(st, tail + off);
    uint8_t blk[128] = {0};
    const size_t rest = tail_len - off, n = rest + 9 <= 64 ? 64 : 128;
    for (size_t i = 0; i < rest; i++) blk[i] = tail[off + i];
    blk[rest] = 0x80;
    const uint64_t bits = 8 * (prefix_bytes + (uint64_t)tail_len);
    for (int i = 0; i < 8; i++) blk[n - 8 + i] = (uint8_t)(bits >> (56 - 8 * i));
    for (size_t o = 0; o < n; o += 64) sha256_compress(st, blk + o);
    sha256_store(st, digest);
}

size_t reveal_mask_bytes(const Circuit &c) { return c.reveal ? TRV_MASK_BYTES(c.message_bytes) : 0; }

size_t mode_header_bytes(const Circuit &c) {
    return c.kind == CIRCUIT_AES_GCM_SEG ? TRS_HDR_BYTES(c.aad_bytes) : c.kind == CIRCUIT_AES_GCM ? 12 + c.aad_bytes : (c.kind == CIRCUIT_AES_CBC || c.kind == CIRCUIT_AES_CTR) ? 16 : 0;
}

size_t segment_header_bytes(const Circuit &c) { return TRS_HDR_DG_BYTES(c.aad_bytes, c.digest_kind) + reveal_mask_bytes(c); }

void gcm_digest_plan_host(const uint8_t *msg, size_t len, const uint8_t *key, size_t key_len, const uint8_t iv[12], const uint8_t *aad, size_t aad_len, size_t c, const uint8_t *h_in, uint64_t prefix,
                          uint8_t *ys, uint8_t *states) {
    if (c == 0 || (16 * c) % 64) throw std::invalid_argument("gcm_digest_plan: a digest segment holds whole 64-byte blocks: c must be a multiple of 4");
    if (len <= 16 * c) throw std::invalid_argument("gcm_digest_plan: this record fits one segment; a record that fits one proof takes a lone GCM key with a final digest (zkaes_synthesize_keys_pd)");
    const size_t nd = (len + 16 * c - 1) / (16 * c);
    // the accumulators behind every data segment but the last are the plain plan's; the one behind the last data block, ahead of the length block, is the chain's end
    gcm_boundaries_host(msg, len, key, key_len, iv, aad, aad_len, c, ys);
    {
        std::vector<uint8_t> ct(len);
        uint8_t tag[16], hb[16] = {0}, blk[16];
        aes128_gcm_encrypt_host(msg, len, key, iv, aad, aad_len, ct.data(), tag, key_len);
        HostAes128 aes(key, key_len);
        aes.encrypt_block(hb);
        const Gf128 h = gf_load(hb);
        Gf128 y = nd > 1 ? gf_load(ys + 16 * (nd - 2)) : Gf128();
        for (size_t off = 16 * c * (nd - 1); off < len; off += 16) {
            for (size_t i = 0; i < 16; i++) blk[i] = off + i < len ? ct[off + i] : 0;
            Gf128 x = gf_load(blk);
            x.hi ^= y.hi; x.lo ^= y.lo;
            y = gf_mul(x, h);
        }
        for (int i = 0; i < 8; i++) { ys[16 * (nd - 1) + i] = (uint8_t)(y.hi >> (56 - 8 * i)); ys[16 * (nd - 1) + 8 + i] = (uint8_t)(y.lo >> (56 - 8 * i)); }
    }
    sha256_chain(h_in, nullptr, 0, states);                                        // states[0] = H_in, null being the initial value
    for (size_t s = 0; s + 1 < nd; s++) sha256_chain(states + 32 * s, msg + 16 * c * s, 16 * c, states + 32 * (s + 1));
    sha256_finish(states + 32 * (nd - 1), prefix + 16 * c * (nd - 1), msg + 16 * c * (nd - 1), len - 16 * c * (nd - 1), states + 32 * nd);
}

}  // namespace zk
