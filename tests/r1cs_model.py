"""A plain model of the layer between the AES trace and the prover's polynomials, on Python integers modulo r: the sparse products, the index maps between variables and
positions on H, round 2's t, the Lagrange-basis scalars, round 3's f and the ChaCha field stream.  Nothing here shares structure with the kernels of
csrc/kernels_witness.hip and csrc/kernels_poly.hip or with the table builder of csrc/marlin_host.hpp: sums run over the CSR matrices entry by entry, no buckets, no
segments, no batches.  tests/test_r1cs_model.py checks it against itself and the CPU oracle; tests/test_gpu_r1cs.py compares the kernels with it byte for byte.

Values are canonical integers in [0, r); pack with the oracle's fr_pack or, for raw Montgomery representatives, poly_model's raw_pack / raw_unpack.  A matrix is a CSR
triple (rowptr, col, coeff) of plain sequences."""
from poly_model import raw_pack, raw_unpack  # noqa: F401  (re-exported: the packing helpers of the polynomial model)

R377 = 0x12ab655e9a2ca55660b44d1e5c37b00159aa76fed00000010a11800000000001
FR_BITS = 253                                          # bit length of r: a candidate's top word keeps its low 253 - 224 bits
TWO_ADICITY, ROOT_OF_UNITY_BASE = 47, 22               # 2^47 | r - 1; 22 generates the multiplicative group (ark-bls12-377 FrParameters::GENERATOR)


def domain_gen(lg, r=R377):
    """the generator of the domain of size 2^lg, as ark-poly's Radix2EvaluationDomain takes it: GENERATOR^((r - 1) / 2^47), squared down"""
    g = pow(ROOT_OF_UNITY_BASE, (r - 1) >> TWO_ADICITY, r)
    for _ in range(lg, TWO_ADICITY):
        g = g * g % r
    return g


# ---- variables <-> positions on H (|H| = n, the instance domain |X| = m, both powers of two, m < n)
def reindex(n, m, i):
    """ark-poly EvaluationDomain::reindex_by_subdomain: variable i (instance first, then witness) -> its position on H"""
    period = n // m
    if i < m:
        return i * period
    j, x = i - m, period - 1
    return j + j // x + 1


def h_map(n, m, k):
    """the inverse as the kernels spell it inline: position k on H -> ("x", instance index) at the multiples of n / m, else ("w", witness index)"""
    ratio = n // m
    if k % ratio == 0:
        return ("x", k // ratio)
    return ("w", k - k // ratio - 1)


def z_on_h(z, n, m, num_witness):
    """the assignment (m instance values then num_witness witness values) at every position of H, witness slots past num_witness zero"""
    out = []
    for k in range(n):
        kind, i = h_map(n, m, k)
        out.append(z[i] if kind == "x" else (z[m + i] if i < num_witness else 0))
    return out


def w_classes(z, n, m, num_witness):
    return [0 if h_map(n, m, k)[0] == "x" else v for k, v in enumerate(z_on_h(z, n, m, num_witness))]


def w_evals(z, x_evals, n, m, num_witness, r=R377):
    """ark-marlin prover_first_round: 0 on X, else w - x_evals"""
    zh = z_on_h(z, n, m, num_witness)
    return [0 if h_map(n, m, k)[0] == "x" else (zh[k] - x_evals[k]) % r for k in range(n)]


# ---- sparse products
def spmv_acc(rowptr, col, coeff, rows, rows_out, z):
    """the INTEGER row sums sum_i coeff[i] z[col[i]], zero for rows <= r < rows_out"""
    out = []
    for r_ in range(rows_out):
        out.append(sum(int(coeff[i]) for i in range(rowptr[r_], rowptr[r_ + 1]) if z[col[i]]) if r_ < rows else 0)
    return out


def spmv(rowptr, col, coeff, rows, rows_out, z, r=R377):
    """(field values, int8 classes clamped to +-127)"""
    acc = spmv_acc(rowptr, col, coeff, rows, rows_out, z)
    return [a % r for a in acc], [max(-127, min(127, a)) for a in acc]


def t_model(n, m, rows, mats, r_alpha, etas, r=R377):
    """t[h] = sum over ALL entries (row, col, c) of A, B, C with reindex(col) = h of eta_M c r_alpha[row], straight from the CSR triples"""
    t = [0] * n
    for (rowptr, col, coeff), eta in zip(mats, etas):
        for row in range(rows):
            for i in range(rowptr[row], rowptr[row + 1]):
                h = reindex(n, m, int(col[i]))
                t[h] = (t[h] + eta * int(coeff[i]) * r_alpha[row]) % r
    return t


# ---- Lagrange-basis scalars at beta
def lagrange(lg_n, lg_m, beta, r=R377):
    """(lag, lag_w): lag[k] = L_k(beta) = (beta^n - 1) g^k / (n (beta - g^k)) -- and 1 where beta = g^k, the value of that polynomial there; lag_w[k] = 0 at the multiples
    of n / m, else L_k(beta) / (beta^m - 1), or None for the whole of lag_w when beta^m = 1 (no inverse: outside the kernel's contract)"""
    n, m, g = 1 << lg_n, 1 << lg_m, domain_gen(lg_n, r)
    vh, n_inv = (pow(beta, n, r) - 1) % r, pow(n, -1, r)
    lag, gk = [], 1
    for _ in range(n):
        lag.append(1 if gk == beta else vh * gk % r * n_inv % r * pow((beta - gk) % r, -1, r) % r)
        gk = gk * g % r
    vx = (pow(beta, m, r) - 1) % r
    if vx == 0:
        return lag, None
    vx_inv = pow(vx, -1, r)
    return lag, [0 if k % (n // m) == 0 else v * vx_inv % r for k, v in enumerate(lag)]


def f_model(va, vb, vc, ea, eb, ec, ra, rb, ri, ci, r=R377):
    """round 3's f on K: (ea va + eb vb + ec vc)[i] rb[ci[i]] ra[ri[i]]"""
    return [(ea * va[i] + eb * vb[i] + ec * vc[i]) * rb[ci[i]] % r * ra[ri[i]] % r for i in range(len(va))]


def mask_fixup(p, n, r=R377):
    """ark-marlin's mask polynomial: p[0] -= p[0] + p[n] + p[2n]"""
    out = list(p)
    out[0] = (p[0] - (p[0] + p[n] + p[2 * n])) % r
    return out


# ---- ChaCha (RFC 7539's quarter round; rand_chacha's layout: 64-bit block counter in words 12-13, words 14-15 zero)
M32 = 0xffffffff


def _rotl(x, n):
    return ((x << n) | (x >> (32 - n))) & M32


def chacha_block(key_words, counter, rounds):
    """the 16 output words of block `counter` (taken modulo 2^64)"""
    s = [0x61707865, 0x3320646e, 0x79622d32, 0x6b206574] + [int(w) for w in key_words] + [counter & M32, (counter >> 32) & M32, 0, 0]
    x = list(s)

    def qr(a, b, c, d):
        x[a] = (x[a] + x[b]) & M32; x[d] = _rotl(x[d] ^ x[a], 16)
        x[c] = (x[c] + x[d]) & M32; x[b] = _rotl(x[b] ^ x[c], 12)
        x[a] = (x[a] + x[b]) & M32; x[d] = _rotl(x[d] ^ x[a], 8)
        x[c] = (x[c] + x[d]) & M32; x[b] = _rotl(x[b] ^ x[c], 7)

    for _ in range(rounds // 2):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    return [(a + b) & M32 for a, b in zip(x, s)]


class WordStream:
    """word w of the key stream = word w % 16 of block w // 16; blocks are computed once"""

    def __init__(self, key_words, rounds):
        self.key, self.rounds, self.blocks = list(key_words), rounds, {}

    def word(self, w):
        b = w // 16
        if b not in self.blocks:
            self.blocks[b] = chacha_block(self.key, b, self.rounds)
        return self.blocks[b][w % 16]


def chacha_words(key_words, rounds, first_word, count):
    ws = WordStream(key_words, rounds)
    return [ws.word(first_word + i) for i in range(count)]


def field_stream(key_words, rounds, word_pos, count, r=R377, bits=FR_BITS):
    """(elements, next_word_pos): a candidate is 8 consecutive words from the current position, little end first, its top word masked to the field's bit length; it is
    accepted iff below r, and its value IS the element's stored (Montgomery) representation -- no conversion.  next_word_pos = the word after the last accepted candidate."""
    ws, out, pos = WordStream(key_words, rounds), [], word_pos
    top_mask = (1 << (bits - 224)) - 1
    while len(out) < count:
        v = 0
        for i in range(8):
            w = ws.word(pos + i)
            v |= (w & top_mask if i == 7 else w) << (32 * i)
        pos += 8
        if v < r:
            out.append(v)
    return out, pos
