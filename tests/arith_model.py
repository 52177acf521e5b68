"""Big-integer model of ONE field or curve operation of csrc/ff.cuh, ff28.cuh, ff29.cuh, ec28.cuh and te28.cuh, and the operand lists the probes of csrc/arith_probe.cuh
are run on: by tests/test_arith_model.py on the host (tests/arith_probe_host.cpp) and by tests/test_gpu_arith.py on the device (zkaes_arith_probe).

Plain Python integers, nothing transliterated from the headers:
  * a limb vector is the integer sum l_i 2^(w i);
  * a Montgomery product of integers A, B is (A B + m p) / R' with m = -A B p^-1 mod R'.  That is exact also for lazy operands: the row-wise reduction's m_i are the base-2^w
    digits of that one m, so the result is determined AS AN INTEGER, and its limbs are that integer's normalized limbs with the excess in the top limb -- the comparison is
    byte equality;
  * additions and subtractions are a + b or a - b + K p, re-limbed by the rule the operation documents (normalized, or limb-wise without carries for the lazy forms, with
    kp_spread derived here from p);
  * the group law is compared AS POINTS: a result is taken back to affine integers (un-Montgomery, divide by Z or ZZ / ZZZ) and compared with tools/curve_math.py.

cases(name) -> list of input word lists (deterministic); check(name, inputs, outputs) asserts everything the model knows about the outputs."""
import functools
import os
import random
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools import curve_math as cm                                           # noqa: E402
from aes_zero_knowledge_proof_circuit_amd.api import ARITH_OPS               # noqa: E402

PRIMES = {"fr377": cm.R377, "fr381": cm.R381, "fq377": cm.Q377, "fq381": cm.Q381}
M32 = 0xffffffff


# ---- limbs and the Montgomery product
def val(limbs, w):
    return sum(l << (w * i) for i, l in enumerate(limbs))


def relimb(v, w, n):
    """normalized limbs of v >= 0, the excess in the top limb"""
    assert v >= 0, "negative value: the operands break the operation's contract"
    out = [(v >> (w * i)) & ((1 << w) - 1) for i in range(n - 1)] + [v >> (w * (n - 1))]
    assert out[-1] <= M32, "the top limb's excess does not fit 32 bits"
    return out


def mont(t, p, rbits):
    """(t + m p) / 2^rbits, m = -t p^-1 mod 2^rbits"""
    r = 1 << rbits
    q, rem = divmod(t + (-t * pow(p, -1, r)) % r * p, r)
    assert rem == 0
    return q


def kp_spread(p, k, w, n):
    """K p as limbs c_i with c_i >= 2^w - 1 below the top: every limb below the top lends 2^w upward and the limb above repays 1"""
    c = relimb(k * p, w, n)
    c = [c[0] + (1 << w)] + [x + (1 << w) - 1 for x in c[1:-1]] + [c[-1] - 1]
    assert val(c, w) == k * p and all(x >= (1 << w) - 1 for x in c[:-1]) and c[-1] >= 0
    return c


class Rep:
    """one limb representation of a field: word size w, n limbs, Montgomery radix 2^(w n)"""

    def __init__(self, p, w, n):
        self.p, self.w, self.n, self.rbits = p, w, n, w * n
        self.mask = (1 << w) - 1
        self.r = (1 << self.rbits) % p

    def val(self, limbs):
        return val(limbs, self.w)

    def limbs(self, v):
        return relimb(v, self.w, self.n)

    def mont(self, t):
        return mont(t, self.p, self.rbits)

    def unmont(self, limbs):
        """the field element a limb vector stands for"""
        return self.val(limbs) * pow(self.r, -1, self.p) % self.p

    def enc(self, x, add_p=0):
        """Montgomery representative of the element x (plus add_p multiples of p), normalized limbs"""
        return self.limbs(x * self.r % self.p + add_p * self.p)

    def maxval(self, bound):
        """the largest value below `bound` whose limbs below the top are all ones"""
        low = (1 << (self.w * (self.n - 1))) - 1
        top = (bound - 1 - low) >> (self.w * (self.n - 1))
        assert top >= 0
        return (top << (self.w * (self.n - 1))) | low


STD = {f: Rep(p, 32, 8 if f.startswith("fr") else 12) for f, p in PRIMES.items()}
X28 = {f + "x28": Rep(PRIMES[f], 28, 14) for f in ("fq377", "fq381")}
X29 = {f + "x29": Rep(PRIMES[f], 29, 9) for f in ("fr377", "fr381")}
MODEL, CASES, CHECK = {}, {}, {}                      # name -> inputs -> outputs | () -> inputs | (inputs, outputs) -> None


# ================================================================ Fp<P>: canonical values, 32-bit limbs, R = 2^(32 N)
def _std_mul(R, a, b):
    r = R.mont(a * b)
    return r - R.p if r >= R.p else r


def _std_specials(R):
    p, bits = R.p, R.p.bit_length()
    s = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, R.r, R.r * R.r % p, (1 << (bits - 1)) - 1, val([M32] * R.n, 32) % (1 << (bits - 1))]
    return s + [1 << k for k in range(0, bits - 1, 7)] + [1 << (bits - 2)]


def _std_register(f):
    R = STD[f]
    p, n = R.p, R.n
    rnd = random.Random("std" + f)
    sp = _std_specials(R)
    rand = [rnd.randrange(p) for _ in range(300)]
    enc = lambda v: relimb(v, 32, n)
    pairs = [(a, b) for a in sp[:12] for b in sp[:12]] + [(a, b) for a in sp[12:] for b in (1, p - 1, sp[12])] + list(zip(rand, rand[1:] + rand[:1]))
    pairs += [(a, p - a) for a in rand[:20] + [1, (p - 1) // 2, p - 1]]                     # a + b lands exactly on p
    pairs += [(p - 1 - a % 5, p - 1 - b % 7) for a, b in zip(rand[:20], rand[20:40])]       # a + b in [p, 2 p)
    # products whose value BEFORE the final conditional subtraction lies in [p, 2 p).  (Exactly p cannot happen for canonical operands: it needs A B = 0 (mod p), hence a zero
    # operand, hence 0.)
    found, tries = [], 0
    while len(found) < 40 and tries < 200000:
        a, b = rnd.randrange(p), rnd.randrange(p)
        tries += 1
        if R.mont(a * b) >= p:
            found.append((a, b))
    assert len(found) == 40, "no product with a pre-subtraction value in [p, 2p) found for " + f
    binops = {"mul": lambda a, b: _std_mul(R, a, b), "add": lambda a, b: (a + b) % p, "sub": lambda a, b: (a - b) % p}
    for op, fn in binops.items():
        MODEL["%s.%s" % (f, op)] = lambda w, fn=fn: enc(fn(val(w[:n], 32), val(w[n:], 32)))
        CASES["%s.%s" % (f, op)] = lambda: [enc(a) + enc(b) for a, b in pairs + found]
    rinv = pow(R.r, -1, p)
    unops = {"neg": lambda a: -a % p, "dbl": lambda a: 2 * a % p, "from_raw": lambda a: a * R.r % p, "to_raw": lambda a: a * rinv % p,
             "inverse": lambda a: pow(a, -1, p) * R.r * R.r % p if a else 0}                # the stored value is x R; the inverse is x^-1 R = R^2 / a
    for op, fn in unops.items():
        MODEL["%s.%s" % (f, op)] = lambda w, fn=fn: enc(fn(val(w, 32)))
        CASES["%s.%s" % (f, op)] = lambda: [enc(a) for a in sp + rand]
    inv_in = [0, R.r, (p - 1) * R.r % p, 2 * R.r % p, (p + 1) // 2 * R.r % p] + [(1 << k) * R.r % p for k in range(2, p.bit_length() + 40, 13)] + [1, 2, p - 1] + rand[:120]
    CASES[f + ".inverse"] = lambda: [enc(a) for a in inv_in]                                # 0, +-1, 2, 1/2, powers of two (as VALUES), raw 1, 2, p - 1
    i64 = [0, 1, -1, 127, -127, -(1 << 63) + 1, (1 << 63) - 1, 1 << 32, -(1 << 32), (1 << 32) - 1] + [rnd.randrange(-(1 << 63) + 1, 1 << 63) for _ in range(100)]
    MODEL[f + ".from_i64"] = lambda w: enc((val(w, 32) - ((val(w, 32) >> 63) << 64)) % p * R.r % p)
    CASES[f + ".from_i64"] = lambda: [relimb(v % (1 << 64), 32, 2) for v in i64]
    exps = [0, 1, 2, 3, (1 << 64) - 1, 1 << 63, 1 << 32, (1 << 32) - 1, 0x5555555555555555] + [rnd.randrange(1 << 64) for _ in range(20)]
    MODEL[f + ".pow_u64"] = lambda w: enc(pow(val(w[:n], 32) * rinv % p, val(w[n:], 32), p) * R.r % p)
    CASES[f + ".pow_u64"] = lambda: [enc(a) + relimb(e, 32, 2) for a in sp[:9] + rand[:12] for e in exps[:9]] + [enc(a) + relimb(e, 32, 2) for a, e in zip(rand[12:32], exps[9:])]


for _f in STD:
    _std_register(_f)


# ================================================================ shared by the reduced-radix forms
def _product_check(R, total):
    """the header's contract for a product of operands inside it (sum of the limb products T <= 0.2 R' p, so that T / R' + p <= 1.2 p): below 1.2 p; always: normalized
    limbs below the top.  total(input words) -> T"""
    def chk(ins, outs):
        for i, o in zip(ins, outs):
            assert all(x <= R.mask for x in o[:-1]), ("limbs not normalized", i, o)
            if total(i) * 5 <= (R.p << R.rbits):
                assert R.val(o) * 10 < 12 * R.p, ("product of operands inside the contract is not below 1.2 p", i, o)
    return chk


def _lazy_vec(rnd, limb_bound, top_bound, n, kind):
    """limb vector with every limb below limb_bound (top below top_bound): 0 = all at the bound - 1, 1 = one below that, 2.. = random close to / anywhere below the bound"""
    out = []
    for i in range(n):
        b = top_bound if i == n - 1 else limb_bound
        out.append(b - 1 if kind == 0 else b - 2 if kind == 1 else b - 1 - rnd.randrange(256 if kind % 2 else b))
    return out


def _reduced_values(R, rnd, bound_p):
    """normalized operands below bound_p x p: the edges and pseudo-random ones"""
    p = R.p
    v = [0, 1, p - 1, p, p + 1, 2 * p, R.r, R.maxval(bound_p * p), R.maxval(p), bound_p * p - 1, R.maxval(1 << (R.w * (R.n - 1)))]
    return v + [rnd.randrange(p) for _ in range(60)] + [rnd.randrange(bound_p * p) for _ in range(60)]


def _sub_lazy_cases(R, rnd, k, lmax):
    """sub_lazy<K>: per limb position b_i in {0, 1, mask - 1, mask, kp_spread_i where that is a limb value} against l_i in {0, lmax}; b's excess in the top limb"""
    sp = kp_spread(R.p, k, R.w, R.n)
    assert all(x != 0 for x in relimb(k * R.p, R.w, R.n)), "a limb of K p is zero: |kp_spread - b| = 0 has one more edge"
    out = []
    for i in range(R.n - 1):
        for bi in [0, 1, R.mask - 1, R.mask] + ([sp[i]] if sp[i] <= R.mask else []):
            for li in (0, lmax):
                a = [rnd.randrange(lmax + 1) for _ in range(R.n)]
                b = [rnd.randrange(R.mask + 1) for _ in range(R.n - 1)] + [rnd.randrange(sp[-1] + 1)]
                a[i], b[i] = li, bi
                out.append(a + b)
    for a_all, b_all in ((0, R.mask), (lmax, R.mask), (0, 0), (lmax, 0), (lmax, 1), (0, R.mask - 1)):        # every limb at once; the top limb of b at its own limits
        for btop in (0, 1, sp[-1] - 1, sp[-1]):
            out.append([a_all] * R.n + [b_all] * (R.n - 1) + [btop])
    for _ in range(200):
        out.append([rnd.randrange(lmax + 1) for _ in range(R.n)] + [rnd.randrange(R.mask + 1) for _ in range(R.n - 1)] + [rnd.randrange(sp[-1] + 1)])
    return out


def _sub_cases(R, rnd, k, left):
    """sub<K>: b normalized with b <= K p (at, just below, low limbs all ones); left operands as given (limb vectors)"""
    p = R.p
    bs = [0, 1, p, k * p, k * p - 1, R.maxval(k * p + 1), R.maxval(p)] + [rnd.randrange(k * p + 1) for _ in range(12)]
    return [a + R.limbs(b) for a in left for b in bs]


# ================================================================ Fp28<P>
def _x28_register(f):
    R, S = X28[f], STD[f[:5]]
    p, n, w = R.p, R.n, R.w
    rnd = random.Random("x28" + f)
    L = R.limbs
    vals = _reduced_values(R, rnd, 64)
    norm = [L(v) for v in vals]
    pairs = [(a, b) for a in norm[:11] for b in norm[:11]] + list(zip(norm[11:], norm[12:] + norm[:1]))
    # ONE lazy operand (limbs <= 5 x 2^28: what sub_lazy<3> of a normalized value leaves) beside a normalized one
    lazy1 = [_lazy_vec(rnd, 5 << 28, 1 << 20, n, k) for k in range(24)]
    pairs += [(a, b) for a in lazy1 for b in (norm[7], norm[8], norm[20], norm[80])] + [(b, a) for a in lazy1[:6] for b in (norm[7], norm[30])]
    hot = []
    if f == "fq377x28":
        # te_madd_hot's widest products: limbs below 4 x 2^28 against 3 x 2^28, top limbs below 2^18 and 2^17 (tests/test_ff28_host.py lazy_bounds), down to one below each
        hot = [(_lazy_vec(rnd, 4 << 28, 1 << 18, n, ka), _lazy_vec(rnd, 3 << 28, 1 << 17, n, kb)) for ka in range(6) for kb in range(6)]
        hot += [(b, a) for a, b in hot[:8]]
    prod = lambda a, b: L(R.mont(R.val(a) * R.val(b)))
    names = ["mul"] + (["mul_biased"] if hot else [])
    for op in names:
        MODEL["%s.%s" % (f, op)] = lambda x: prod(x[:n], x[n:])
        CASES["%s.%s" % (f, op)] = lambda: [a + b for a, b in pairs + hot]
        CHECK["%s.%s" % (f, op)] = _product_check(R, lambda x: R.val(x[:n]) * R.val(x[n:]))
    MODEL[f + ".sqr"] = lambda x: prod(x, x)
    CASES[f + ".sqr"] = lambda: norm
    CHECK[f + ".sqr"] = _product_check(R, lambda x: R.val(x) ** 2)
    # fma2: a b + c d < 64 p^2 (operands below 5.6 p), normalized
    small = [L(v) for v in [0, 1, p, p - 1, R.maxval(5 * p), R.maxval(p), 5 * p + p // 2] + [rnd.randrange(5 * p) for _ in range(40)]]
    quads = [(a, b, c, d) for a in small[:6] for b in small[:6] for c in (small[1], small[4]) for d in (small[3], small[4])]
    quads += [tuple(small[(i + j) % len(small)] for j in (0, 3, 7, 11)) for i in range(len(small))]
    quads += [(L(a), L(b), L(p - a), L(b)) for a, b in ((rnd.randrange(1, p), rnd.randrange(1, p)) for _ in range(10))]          # a b + (p - a) b = p b: reduces to exactly p
    MODEL[f + ".fma2"] = lambda x: L(R.mont(R.val(x[:n]) * R.val(x[n:2 * n]) + R.val(x[2 * n:3 * n]) * R.val(x[3 * n:])))
    CASES[f + ".fma2"] = lambda: [a + b + c + d for a, b, c, d in quads]
    CHECK[f + ".fma2"] = _product_check(R, lambda x: R.val(x[:n]) * R.val(x[n:2 * n]) + R.val(x[2 * n:3 * n]) * R.val(x[3 * n:]))
    half = [L(v) for v in _reduced_values(R, rnd, 32)]
    MODEL[f + ".add"] = lambda x: L(R.val(x[:n]) + R.val(x[n:]))
    CASES[f + ".add"] = lambda: [a + b for a in half[:11] for b in half[:11]] + [a + b for a, b in zip(half[11:], half[12:] + half[:1])]
    lazy_in = [a + b for a, b in zip(lazy1, lazy1[1:] + lazy1[:1])] + [a + b for a in norm[:11] for b in norm[:11]]
    MODEL[f + ".add_lazy"] = lambda x: [(a + b) & M32 for a, b in zip(x[:n], x[n:])]
    CASES[f + ".add_lazy"] = lambda: lazy_in
    MODEL[f + ".dbl_lazy"] = lambda x: [(a << 1) & M32 for a in x]
    CASES[f + ".dbl_lazy"] = lambda: norm + [_lazy_vec(rnd, 1 << 31, 1 << 20, n, k) for k in range(8)]
    for k in (2, 3, 4, 5, 6, 7):
        MODEL["%s.sub%d" % (f, k)] = lambda x, k=k: L(R.val(x[:n]) - R.val(x[n:]) + k * p)
        CASES["%s.sub%d" % (f, k)] = lambda k=k: _sub_cases(R, random.Random("sub%d" % k + f), k, norm[:12] + norm[40:60] + norm[100:110])
    for k in (2, 3):
        sp = kp_spread(p, k, w, n)
        MODEL["%s.sub_lazy%d" % (f, k)] = lambda x, sp=sp: [(a + c - b) & M32 for a, b, c in zip(x[:n], x[n:], sp)]
        CASES["%s.sub_lazy%d" % (f, k)] = lambda k=k: _sub_lazy_cases(R, random.Random("subl%d" % k + f), k, (k + 2) << 28)
    kp = [L(v) for k in range(64) for v in (k * p - 1, k * p, k * p + 1) if 0 <= v < 64 * p] + [L(R.maxval(64 * p)), L(64 * p - 1)] + norm[11:71]
    MODEL[f + ".canonical"] = lambda x: L(R.val(x) % p)
    MODEL[f + ".is_zero_mod_p"] = lambda x: [1 if R.val(x) % p == 0 else 0]
    CASES[f + ".canonical"] = CASES[f + ".is_zero_mod_p"] = lambda: kp
    # product_is_zero: v in {0, p} as LIMBS; one limb of p flipped in each position; limb 0 = p_0 with another limb off; limb 0 = 0 with another limb set
    pl, piz = L(p), [L(0), L(p)]
    for i in range(n):
        for d in (1, -1):
            piz.append([x + d if j == i else x for j, x in enumerate(pl)])
        if i:
            piz.append([pl[0]] + [1 if j == i else 0 for j in range(1, n)])
            piz.append([0] + [1 if j == i else 0 for j in range(1, n)])
            piz.append([0] + pl[1:i] + [pl[i] ^ 1] + pl[i + 1:])
    piz += [x for x in norm[11:40] if all(y <= R.mask for y in x[:-1]) and R.val(x) * 10 < 12 * p]
    MODEL[f + ".product_is_zero"] = lambda x: [1 if x in (L(0), pl) else 0]
    CASES[f + ".product_is_zero"] = lambda: [[x & M32 for x in v] for v in piz if all(x >= 0 for x in v)]
    k400, k384 = (1 << 400) % p, (1 << 384) % p
    sv = _std_specials(S) + [rnd.randrange(p) for _ in range(150)]
    MODEL[f + ".from_std"] = lambda x: L(R.mont(val(x, 32) * k400))
    CASES[f + ".from_std"] = lambda: [relimb(v, 32, 12) for v in sv]
    CHECK[f + ".from_std"] = _product_check(R, lambda x: val(x, 32) * k400)
    MODEL[f + ".to_std"] = lambda x: relimb(R.mont(R.val(x) * k384) % p, 32, 12)
    CASES[f + ".to_std"] = lambda: norm


for _f in X28:
    _x28_register(_f)


# ================================================================ Fp29<P>
def reduce_by_top_limb_model(R, v):
    """v - floor(l_8 RECIP / 2^32) p with RECIP = floor(2^32 / (p_8 + 1)), l_8 and p_8 the top limbs of v and p"""
    sh = R.w * (R.n - 1)
    recip = (1 << 32) // ((R.p >> sh) + 1)
    return v - (((v >> sh) * recip) >> 32) * R.p


def _x29_register(f):
    R, S = X29[f], STD[f[:5]]
    p, n, w = R.p, R.n, R.w
    rnd = random.Random("x29" + f)
    L = R.limbs
    vals = _reduced_values(R, rnd, 32)
    norm = [L(v) for v in vals]
    canon = [L(v) for v in [0, 1, p - 1, R.maxval(p), R.r] + [rnd.randrange(p) for _ in range(40)]]
    # a < B p beside a canonical b (the header's contract), and ONE lazy operand with limbs below 6 x 2^29 beside a normalized one
    pairs = [(a, b) for a in norm[:11] + norm[40:70] + norm[100:130] for b in canon[:5] + canon[10:13]]
    lazy1 = [_lazy_vec(rnd, 6 << 29, 1 << 26, n, k) for k in range(24)]
    pairs += [(a, b) for a in lazy1 for b in canon[:5] + canon[20:23]] + [(b, a) for a in lazy1[:6] for b in canon[2:5]]
    MODEL[f + ".mul"] = lambda x: L(R.mont(R.val(x[:n]) * R.val(x[n:])))
    CASES[f + ".mul"] = lambda: [a + b for a, b in pairs]
    # dot<M>: a[i] < 4 p, b[i] < 2 p (kernels_poly.hip's operands), every term at its bound, limbs all ones; one term non-zero; terms that cancel to 0 and to p
    a4 = [L(v) for v in [R.maxval(4 * p), 4 * p - 1, 0, p, 1] + [rnd.randrange(4 * p) for _ in range(30)]]
    b2 = [L(v) for v in [R.maxval(2 * p), 2 * p - 1, 0, p - 1, 1] + [rnd.randrange(2 * p) for _ in range(30)]]
    for m in (2, 3, 4):
        cs = [[a4[0]] * m + [b2[0]] * m, [a4[1]] * m + [b2[1]] * m, [a4[0]] * m + [b2[1]] * m, [a4[2]] * 2 * m]
        for t in range(m):                                  # one term non-zero
            for a, b in ((a4[0], b2[0]), (a4[7], b2[9])):
                cs.append([a if i == t else L(0) for i in range(m)] + [b if i == t else L(0) for i in range(m)])
        for _ in range(10):                                 # a b + (p - a) b (+ zeros) = p b: reduces to exactly p; with b = 0 to 0
            a, b = rnd.randrange(1, p), rnd.randrange(1, 2 * p)
            cs.append([L(a), L(p - a)] + [L(0)] * (m - 2) + [L(b), L(b)] + [L(rnd.randrange(p)) for _ in range(m - 2)])
            cs.append([L(a), L(p - a)] + [L(0)] * (m - 2) + [L(0)] * m)
        for i in range(60):
            cs.append([a4[(i + 3 * j) % len(a4)] for j in range(m)] + [b2[(i + 5 * j) % len(b2)] for j in range(m)])
        MODEL["%s.dot%d" % (f, m)] = lambda x, m=m: L(R.mont(sum(R.val(x[i * n:(i + 1) * n]) * R.val(x[(m + i) * n:(m + i + 1) * n]) for i in range(m))))
        CASES["%s.dot%d" % (f, m)] = lambda cs=cs: [sum(c, []) for c in cs]
        # the header's bound (sum A_i B_i / 256 + 1) p, A = 4, B = 2, rests on p / R' < 2^-8: BLS12-377's scalar field (the only one the kernels take dot<> of)
        CHECK["%s.dot%d" % (f, m)] = lambda ins, outs, m=m: [_assert(all(x <= R.mask for x in o[:-1]) and (p << 8 > 1 << R.rbits or R.val(o) * 256 < (8 * m + 256) * p), ("dot out of its bound", o)) for o in outs]
    # operator+ and sub<K> take a lazy LEFT operand with limbs below 5 x 2^29 and return normalized limbs
    lazy5 = [_lazy_vec(rnd, 5 << 29, 1 << 26, n, k) for k in range(12)]
    half = [L(v) for v in _reduced_values(R, rnd, 16)]
    MODEL[f + ".add"] = lambda x: L(R.val(x[:n]) + R.val(x[n:]))
    CASES[f + ".add"] = lambda: [a + b for a in half[:11] + lazy5 for b in half[:11]] + [a + b for a, b in zip(half[11:], half[12:] + half[:1])]
    MODEL[f + ".add_lazy"] = lambda x: [(a + b) & M32 for a, b in zip(x[:n], x[n:])]
    CASES[f + ".add_lazy"] = lambda: [a + b for a in lazy5 + norm[:11] for b in norm[:11]]
    for k in (1, 2, 4, 8):
        MODEL["%s.sub%d" % (f, k)] = lambda x, k=k: L(R.val(x[:n]) - R.val(x[n:]) + k * p)
        CASES["%s.sub%d" % (f, k)] = lambda k=k: _sub_cases(R, random.Random("sub%d" % k + f), k, half[:12] + half[40:60] + lazy5)
    sp = kp_spread(p, 2, w, n)
    MODEL[f + ".sub_lazy2"] = lambda x: [(a + c - b) & M32 for a, b, c in zip(x[:n], x[n:], sp)]
    CASES[f + ".sub_lazy2"] = lambda: _sub_lazy_cases(R, random.Random("subl2" + f), 2, 5 << 29)
    # normalized(): lazy limbs, each anywhere below 2^32 except that the value must leave the top limb room for the carry
    nz = [[M32] * (n - 1) + [0], [M32] * (n - 1) + [M32 - 8], [0] * n, [R.mask + 1] * n] + lazy1 + [[rnd.randrange(1 << 32) for _ in range(n - 1)] + [rnd.randrange(1 << 31)] for _ in range(200)]
    MODEL[f + ".normalized"] = lambda x: L(R.val(x))
    CASES[f + ".normalized"] = lambda: nz
    below256 = [L(v) for v in [0, 1, p, (1 << 256) - 1, 1 << 255, R.maxval(1 << 256), R.maxval(p)] + [rnd.randrange(1 << 256) for _ in range(100)]]
    MODEL[f + ".shl5"] = lambda x: L(R.val(x) << 5)
    CASES[f + ".shl5"] = lambda: below256
    for lg in (0, 1, 4):
        top = 2 << lg
        kp = [L(v) for k in range(top + 1) for v in (k * p - 1, k * p, k * p + 1) if 0 <= v < top * p] + [L(rnd.randrange(top * p)) for _ in range(100)]
        MODEL["%s.canonical%d" % (f, lg)] = lambda x: L(R.val(x) % p)
        CASES["%s.canonical%d" % (f, lg)] = lambda kp=kp: kp
    # reduce_by_top_limb: K p - 1, K p, K p + 1 for K = 0 .. 32 below 32 p, the largest and smallest top limb of every [K p, (K + 1) p) with the limbs under it all zeros
    # and all ones, 32 p - 1, pseudo-random v < 32 p
    sh = w * (n - 1)
    rv = {v for k in range(33) for v in (k * p - 1, k * p, k * p + 1)}
    for k in range(32):
        for t in ((k * p) >> sh, ((k + 1) * p - 1) >> sh):
            rv |= {t << sh, (t << sh) | ((1 << sh) - 1), ((t + 1) << sh) - 1 - (1 << (sh - 1))}
    rv = sorted(v for v in rv if 0 <= v < 32 * p) + [rnd.randrange(32 * p) for _ in range(1500)]
    assert 32 * p - 1 in rv
    MODEL[f + ".reduce_by_top_limb"] = lambda x: L(reduce_by_top_limb_model(R, R.val(x)))
    CASES[f + ".reduce_by_top_limb"] = lambda: [L(v) for v in rv]

    def chk_reduce(ins, outs):
        for i, o in zip(ins, outs):
            v = R.val(o)
            assert all(x <= R.mask for x in o[:-1]) and v * 100 < 107 * p and v < 1 << 256 and v % p == R.val(i) % p, ("reduce_by_top_limb out of its bound", i, o)
    CHECK[f + ".reduce_by_top_limb"] = chk_reduce
    reduced = [L(reduce_by_top_limb_model(R, v)) for v in rv[:400]]
    CASES[f + ".canonical0"] = lambda kp=CASES[f + ".canonical0"](): kp + reduced                 # ... then canonical<0> of the remainders
    tw = _std_specials(S) + [rnd.randrange(p) for _ in range(100)]
    MODEL[f + ".twiddle_from_std"] = lambda x: L((val(x, 32) << 5) % p)
    CASES[f + ".twiddle_from_std"] = lambda: [relimb(v, 32, 8) for v in tw]
    w256 = [0, 1, p - 1, (1 << 256) - 1, 0x5555 * ((1 << 256) // 0xffff)] + [1 << k for k in range(0, 256, 9)] + [rnd.randrange(1 << 256) for _ in range(100)]
    MODEL[f + ".split"] = lambda x: L(val(x, 32))
    CASES[f + ".split"] = lambda: [relimb(v, 32, 8) for v in w256]
    MODEL[f + ".pack"] = lambda x: relimb(R.val(x), 32, 8)
    CASES[f + ".pack"] = lambda: [L(v) for v in w256] + reduced                                    # ... and the pack / split round trip of the remainders


def _assert(ok, what):
    assert ok, what


for _f in X29:
    _x29_register(_f)


# ================================================================ the group law, compared as points
Q = cm.Q377
TE = cm.edwards_377()
G377 = X28["fq377x28"]
SCALARS = [1, 2, 3, 5, 7, 0x1234, (1 << 48) - 1, 0x8000_0000_0001, 0xdead_beef_cafe, 0x1357_9bdf_2468]


@functools.lru_cache(maxsize=None)
def wpoint(curve, k):
    """k G on the Weierstrass model (None = infinity); negative k = the negative"""
    g, q = (cm.G1_377, cm.Q377) if curve == 377 else (cm.G1_381, cm.Q381)
    pt = cm.ec_mul(abs(k), g, q)
    return pt if k >= 0 or pt is None else (pt[0], -pt[1] % q)


def wneg(pt, q):
    return None if pt is None else (pt[0], -pt[1] % q)


def te_affine(k):
    return cm.te_from_weierstrass(wpoint(377, k), TE)


def _pick_rep(R, x, rnd, bound10):
    """a representative of the Montgomery value of x: canonical, or + p where that stays inside the coordinate's bound (bound10 / 10 x p)"""
    v = x * R.r % R.p
    if rnd.random() < 0.5 and (v + R.p) * 10 < bound10 * R.p:
        v += R.p
    return R.limbs(v)


def te_enc(E, rnd, z=None):
    """extended coordinates (X : Y : Z : T) of an affine Edwards point with a pseudo-random Z (z = 1: as te_identity / a fresh accumulator holds it), each coordinate a
    representative below 1.2 p"""
    x, y = E
    z = z or rnd.randrange(1, Q)
    return sum((_pick_rep(G377, c, rnd, 12) for c in (x * z % Q, y * z % Q, z, x * y * z % Q)), [])


def te_dec(words):
    """(affine Edwards point, T consistent with X Y / Z)"""
    X, Y, Z, T = (G377.unmont(words[14 * i:14 * i + 14]) for i in range(4))
    assert Z % Q, "Z = 0"
    zi = pow(Z, -1, Q)
    return (X * zi % Q, Y * zi % Q), (T * Z - X * Y) % Q == 0


def niels_enc(E, R=G377):
    x, y = E
    return sum((R.limbs(c % Q * R.r % Q) for c in (y - x, y + x, TE["k2d"] * x * y)), [])


NIELS_IDENTITY = niels_enc((0, 1))
# te_identity() limb for limb: x and t are all-zero limbs.  te_neg used to return 2 p - 0 = 2 p for them, ON the bound its header states (below 2 p), not below it.
NEG_OF_EXACT_ZERO = [0] * 14 + G377.limbs(G377.r) * 2 + [0] * 14


def _te_outputs_ok(outs, ncoord=4, bound10=12):
    for o in outs:
        for i in range(ncoord):
            c = o[14 * i:14 * i + 14]
            assert all(x <= G377.mask for x in c[:-1]) and G377.val(c) * 10 < bound10 * Q, ("coordinate out of its bound", i, c)


def _te_register():
    rnd = random.Random("te377")
    ks = SCALARS
    pts = {k: te_affine(k) for k in ks + [-k for k in ks] + [0] + [2 * k for k in ks] + [a + b for a in ks for b in ks] + [a - b for a in ks for b in ks]}
    want_w = {}

    # ---- te_madd: acc (any representative, any Z) + table record; P + P, P + (-P), identity on either side and on both
    madd = [(a, b) for a in ks[:6] + [0] for b in ks[:6] + [0]] + [(a, -a) for a in ks] + [(a, a) for a in ks] + [(-a, b) for a, b in zip(ks, ks[1:])]
    madd_in = [te_enc(pts[a], rnd, 1 if a == 0 and i % 2 else None) + niels_enc(pts[b]) for i, (a, b) in enumerate(madd)]
    CASES["te377.te_madd"] = lambda: madd_in

    def chk_sum(pairs, name):
        def chk(ins, outs):
            _te_outputs_ok(outs)
            for (a, b), o in zip(pairs, outs):
                got, t_ok = te_dec(o)
                assert got == te_affine(a + b) and t_ok, (name, a, b)
        return chk
    CHECK["te377.te_madd"] = chk_sum(madd, "te_madd")
    add_in = [te_enc(pts[a], rnd, 1 if a == 0 and i % 2 else None) + te_enc(pts[b], rnd, 1 if b == 0 and i % 3 else None) for i, (a, b) in enumerate(madd)]
    for op in ("te_add", "te_add_quad"):
        CASES["te377." + op] = lambda: add_in
        CHECK["te377." + op] = chk_sum(madd, op)
    dbl = ks + [-k for k in ks] + [a + b for a in ks[:7] for b in ks[:7]] + [0, 0, 0]      # 72 cases: more than one wave of quads, the last one partly idle
    dbl_in = [te_enc(pts[a], rnd, 1 if a == 0 and i % 2 else None) for i, a in enumerate(dbl)]
    dbl_in[-1] = NEG_OF_EXACT_ZERO
    for op in ("te_dbl", "te_dbl_quad"):
        CASES["te377." + op] = lambda: dbl_in
        CHECK["te377." + op] = chk_sum([(a, a) for a in dbl], op)
    CASES["te377.te_neg"] = lambda: dbl_in

    def chk_neg(ins, outs):
        _te_outputs_ok(outs, bound10=20)
        for a, i, o in zip(dbl, ins, outs):
            got, t_ok = te_dec(o)
            assert got == te_affine(-a) and t_ok and o[14:42] == i[14:42], ("te_neg", a)
    CHECK["te377.te_neg"] = chk_neg
    CASES["te377.te_to_std_point"] = lambda: dbl_in

    def xyzz_dec(o, S):
        x, y, zz, zzz = (val(o[12 * i:12 * i + 12], 32) for i in range(4))
        assert max(x, y, zz, zzz) < S.p, "non-canonical standard-form coordinate"
        if zz == 0:
            assert o == [0] * 48, "infinity must be all zero"
            return None
        x, y, zz, zzz = (S.unmont(relimb(c, 32, 12)) for c in (x, y, zz, zzz))
        assert (zz ** 3 - zzz ** 2) % S.p == 0
        return (x * pow(zz, -1, S.p) % S.p, y * pow(zzz, -1, S.p) % S.p)

    def chk_to_std(ins, outs):
        for a, o in zip(dbl, outs):
            assert xyzz_dec(o, STD["fq377"]) == wpoint(377, a), ("te_to_std_point", a)
    CHECK["te377.te_to_std_point"] = chk_to_std
    # ---- niels_from_weierstrass: subgroup points, infinity (0, 0) -> the identity record, the two-torsion point (-1, 0) -> bad
    S = STD["fq377"]
    nfw = ks + [-k for k in ks[:4]] + [0, "torsion"]
    aff = lambda pt: relimb(pt[0] * S.r % Q, 32, 12) + relimb(pt[1] * S.r % Q, 32, 12)
    CASES["te377.niels_from_weierstrass"] = lambda: [aff((Q - 1, 0)) if k == "torsion" else [0] * 24 if k == 0 else aff(wpoint(377, k)) for k in nfw]

    def chk_nfw(ins, outs):
        k400 = (1 << 400) % Q
        for k, o in zip(nfw, outs):
            assert o[42] == (1 if k == "torsion" else 0), ("bad flag", k)
            if k in (0, "torsion"):
                assert o[:42] == NIELS_IDENTITY, ("identity record", k)
                continue
            x, y = te_affine(k)
            # from_std of a CANONICAL standard-form value is one determined integer
            want = sum((G377.limbs(G377.mont(c % Q * S.r % Q * k400)) for c in (y - x, y + x, TE["k2d"] * x * y)), [])
            assert o[:42] == want, ("niels_from_weierstrass", k)
    CHECK["te377.niels_from_weierstrass"] = chk_nfw


_te_register()


# te_madd_hot: chains of seven additions with mixed signs, checked after every step.  One call of hot_step_cases per step; the accumulators of step s are the outputs of s - 1.
HOT_CHAINS = []
_r = random.Random("hot")
for _c in range(24):
    _ks = [_r.choice(SCALARS) for _ in range(8)]
    if _c == 0:
        _ks = [SCALARS[3]] * 8                                  # the same point again and again, from the identity
    _negs = [bool((_c >> s) & 1) if _c < 16 else _r.random() < 0.5 for s in range(8)]
    if _c < 4:
        _negs = [bool(_c & 1), bool(_c & 2)] + _negs[2:]        # both signs of the current digit x both signs of the next one at step 0
    if _c == 0:
        _negs = [False, False, False, True, True, True, True, False]      # P, 2 P (P + P), 3 P, 2 P, P, the identity (P - P), -P
    HOT_CHAINS.append((_c % 3 and _r.choice(SCALARS) or 0, _ks, _negs))      # (start: k G or the identity, points, signs)


def hot_step_cases(step, prev_out=None):
    """inputs of step `step` (0..6) of every chain; prev_out = the outputs of step - 1"""
    rnd = random.Random("hotstep%d" % step)
    ins = []
    for c, (start, ks, negs) in enumerate(HOT_CHAINS):
        acc = te_enc(te_affine(start), rnd, 1 if start == 0 else None) if step == 0 else prev_out[c][:56]
        rec, nxt = niels_enc(te_affine(ks[step])), niels_enc(te_affine(ks[step + 1]))
        cur = rec[14:28] + rec[:14] + rec[28:] if negs[step] else rec                   # as niels_load_signed leaves it
        if step:
            assert prev_out[c][56:] == cur, "the record te_madd_hot left in n is not the next record loaded with its sign"
        ins.append(acc + cur + nxt + [int(negs[step]), int(negs[step + 1])])
    return ins


def hot_step_check(step, outs):
    _te_outputs_ok(outs)
    for (start, ks, negs), o in zip(HOT_CHAINS, outs):
        want = start + sum(-k if s else k for k, s in zip(ks[:step + 1], negs[:step + 1]))
        got, t_ok = te_dec(o)
        assert got == te_affine(want) and t_ok, ("te_madd_hot", step, start, ks, negs)
        nxt = niels_enc(te_affine(ks[step + 1]))
        assert o[56:] == (nxt[14:28] + nxt[:14] + nxt[28:] if negs[step + 1] else nxt), ("record left in n", step)


def hot_as_madd(ins):
    """te_madd inputs that must give the SAME BYTES as te_madd_hot for a positive digit (every factor is the same integer in another limb layout); None where neg"""
    return [None if i[140] else i[:98] for i in ins]


# ---- the Weierstrass law on reduced-radix XYZZ points (both curves)
def _w_register(curve):
    f, q = "w%d" % curve, (cm.Q377 if curve == 377 else cm.Q381)
    R, S = X28["fq%dx28" % curve], STD["fq%d" % curve]
    rnd = random.Random(f)
    ks = SCALARS

    def acc_enc(pt, bx=62, by=32):
        """XYZZ accumulator of an affine point with a pseudo-random Z: x < 6.2 p, y < 3.2 p, zz, zzz < 1.2 p; None -> all zero"""
        if pt is None:
            return [0] * 56
        z = rnd.randrange(1, q)
        reps = []
        for c, b10 in ((pt[0] * z * z, bx), (pt[1] * z ** 3, by), (z * z, 12), (z ** 3, 12)):
            v = c % q * R.r % q
            v += rnd.randrange((b10 * q // 10 - v) // q + 1) * q
            reps.append(R.limbs(v))
        return sum(reps, [])

    def acc_dec(o):
        x, y, zz, zzz = (o[14 * i:14 * i + 14] for i in range(4))
        if zz == [0] * 14:
            return None
        x, y, zz, zzz = (R.unmont(c) for c in (x, y, zz, zzz))
        assert zz % q and (zz ** 3 - zzz ** 2) % q == 0, "zz^3 != zzz^2"
        return (x * pow(zz, -1, q) % q, y * pow(zzz, -1, q) % q)

    def bounds(outs, bx, by):
        for o in outs:
            for i, b10 in enumerate((bx, by, 12, 12)):
                c = o[14 * i:14 * i + 14]
                assert all(x <= R.mask for x in c[:-1]) and R.val(c) * 10 < b10 * q, ("coordinate out of its bound", i, c)

    W = lambda k: wpoint(curve, k)
    aff28 = lambda pt: R.enc(pt[0]) + R.enc(pt[1])
    madd = [(a, b) for a in ks[:6] for b in ks[:6]] + [(a, -a) for a in ks] + [(-a, b) for a, b in zip(ks, ks[1:])]
    madd_in = [acc_enc(W(a)) + aff28(W(b)) for a, b in madd]
    CASES[f + ".madd28"] = lambda: madd_in

    def chk_madd(ins, outs):
        for (a, b), i, o in zip(madd, ins, outs):
            if abs(a) == abs(b):                                                          # P = +-Q: refused, the accumulator untouched
                assert o[56] == 0 and o[:56] == i[:56], ("madd28 must refuse P = +-Q", a, b)
            else:
                assert o[56] == 1 and acc_dec(o[:56]) == W(a + b), ("madd28", a, b)
                bounds([o], 62, 12)
    CHECK[f + ".madd28"] = chk_madd
    add = [(a, b) for a in ks[:6] + [0] for b in ks[:6] + [0]] + [(a, -a) for a in ks] + [(a, a) for a in ks] + [(-a, b) for a, b in zip(ks, ks[1:])]
    add_in = [acc_enc(W(a), by=40) + acc_enc(W(b), by=40) for a, b in add]
    CASES[f + ".add28"] = lambda: add_in
    CHECK[f + ".add28"] = lambda ins, outs: [_assert(acc_dec(o) == W(a + b), ("add28", a, b)) for (a, b), o in zip(add, outs)]
    one = ks + [-k for k in ks] + [0]
    one_in = [acc_enc(W(a), by=40) for a in one]
    for op in ("dbl28", "neg28", "to_std_point"):
        CASES["%s.%s" % (f, op)] = lambda: one_in
    CHECK[f + ".dbl28"] = lambda ins, outs: [_assert(acc_dec(o) == W(2 * a), ("dbl28", a)) for a, o in zip(one, outs)] + [bounds([o for a, o in zip(one, outs) if a], 42, 32)]
    CHECK[f + ".neg28"] = lambda ins, outs: [_assert(acc_dec(o) == W(-a) and o[:14] == i[:14] and o[28:] == i[28:], ("neg28", a)) for a, i, o in zip(one, ins, outs)]

    def chk_std(ins, outs):
        for a, o in zip(one, outs):
            x, y, zz, zzz = (val(o[12 * i:12 * i + 12], 32) for i in range(4))
            assert max(x, y, zz, zzz) < q, "non-canonical standard-form coordinate"
            if a == 0:
                assert o == [0] * 48
                continue
            x, y, zz, zzz = (c * pow(S.r, -1, q) % q for c in (x, y, zz, zzz))
            assert (x * pow(zz, -1, q) % q, y * pow(zzz, -1, q) % q) == W(a), ("to_std_point", a)
    CHECK[f + ".to_std_point"] = chk_std


_w_register(377)
_w_register(381)

HOT = "te377.te_madd_hot"
assert set(MODEL) | set(CHECK) | {HOT} == set(ARITH_OPS), sorted(set(ARITH_OPS) ^ (set(MODEL) | set(CHECK) | {HOT}))
assert set(CASES) | {HOT} == set(ARITH_OPS)


@functools.lru_cache(maxsize=None)
def cases(name):
    c = CASES[name]()
    nin = ARITH_OPS[name][1]
    assert 0 < len(c) <= 4096 and all(len(x) == nin and all(0 <= w <= M32 for w in x) for x in c), name
    return c


@functools.lru_cache(maxsize=None)
def expected(name):
    """the model's outputs for cases(name), computed once and shared by the host and the device tests (None: the operation is checked as points only)"""
    return [MODEL[name](list(x)) for x in cases(name)] if name in MODEL else None


def pack(case_list):
    return b"".join(struct.pack("<%dI" % len(c), *c) for c in case_list)


def unpack(buf, nout):
    words = struct.unpack("<%dI" % (len(buf) // 4), buf)
    return [list(words[i:i + nout]) for i in range(0, len(words), nout)]


def check(name, ins, outs):
    """outs: output word lists of cases(name) from the host or the device"""
    assert len(outs) == len(ins)
    want = expected(name) if ins is cases(name) else ([MODEL[name](list(x)) for x in ins] if name in MODEL else None)
    if want is not None:
        bad = [i for i in range(len(ins)) if outs[i] != want[i]]
        assert not bad, "%s: %d of %d cases differ from the model; first: in %s, got %s, want %s" % (
            name, len(bad), len(ins), [hex(x) for x in ins[bad[0]]], [hex(x) for x in outs[bad[0]]], [hex(x) for x in want[bad[0]]])
    if name in CHECK:
        CHECK[name](ins, outs)
