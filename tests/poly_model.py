"""A plain model of the prover's polynomial layer on Python integers modulo r: schoolbook recurrences, no blocking, nothing shared with the structure of the kernels in
csrc/kernels_poly.hip.  tests/test_poly_model.py checks it against itself and against the CPU oracle; tests/test_gpu_poly.py compares the kernels with it byte for byte.

Values are canonical integers in [0, r).  The LINEAR operations (division by X - z or X^m - 1, evaluation, linear combination, coset scaling, the transform) also accept the
raw Montgomery representatives of their data -- x R mod r with R = 2^256 -- because a linear map of R x is R times the map of x: raw_unpack / raw_pack skip the two
conversions, which cost more than the arithmetic."""

R_MONT = 1 << 256


def raw_unpack(buf):
    """32-byte little-endian words -> integers, NO Montgomery conversion"""
    return [int.from_bytes(buf[i:i + 32], "little") for i in range(0, len(buf), 32)]


def raw_pack(vals):
    return b"".join(v.to_bytes(32, "little") for v in vals)


def divide_by_linear(p, z, r):
    """(q, p(z)) with p = q (X - z) + p(z):  q_i = p_(i+1) + z q_(i+1)"""
    q, carry = [0] * max(len(p) - 1, 0), 0
    for i in range(len(p) - 1, 0, -1):
        carry = (p[i] + z * carry) % r
        q[i - 1] = carry
    return q, ((p[0] + z * carry) % r if p else 0)


def divide_by_vanishing(p, m, r):
    """(q, rem) with p = q (X^m - 1) + rem, deg rem < m:  q_i = p_(i+m) + q_(i+m), rem_j = p_j + q_j, residue class by residue class"""
    n = len(p)
    assert n > m >= 1
    q = [0] * (n - m)
    for i in range(n - m - 1, -1, -1):
        q[i] = (p[i + m] + (q[i + m] if i + m < n - m else 0)) % r
    rem = [((p[j] if j < n else 0) + (q[j] if j < n - m else 0)) % r for j in range(m)]
    return q, rem


def horner(p, x, r):
    acc = 0
    for c in reversed(p):
        acc = (acc * x + c) % r
    return acc


def poly_mul(a, b, r):
    out = [0] * (len(a) + len(b) - 1) if a and b else []
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] = (out[i + j] + x * y) % r
    return out


def inverse_mismatch(xs, ys, r, post=1, unit=1):
    """first index where ys[i] is not post / xs[i] (zeros must stay zero), or None.  The inverse is DEFINED by x y == 1 and checked by multiplying back.  With raw Montgomery
    representatives on both sides pass unit = R^2 mod r (x R * y R = x y R^2) and the true value of post."""
    want = post * unit % r
    for i, (x, y) in enumerate(zip(xs, ys)):
        if x == 0:
            if y != 0:
                return i
        elif x * y % r != want:
            return i
    return None


def lincomb(polys, scalars, n, r):
    out = [0] * n
    for p, s in zip(polys, scalars):
        for i, c in enumerate(p[:n]):
            out[i] = (out[i] + s * c) % r
    return out


def vq_holds(out, a, y, n, r, unit=1):
    """is out == r(a, y) = (a^n - y^n) / (a - y)?  Checked WITHOUT a division: out (a - y) == a^n - y^n, and n a^(n-1) where a == y (the quotient's value there).
    unit = R mod r compares a raw Montgomery representative of out."""
    if (a - y) % r == 0:
        return out % r == n * pow(a, n - 1, r) * unit % r
    return out * (a - y) % r == (pow(a, n, r) - pow(y, n, r)) * unit % r


def vq_product(a, y, lg_n, r):
    """the product formula prod_(k < lg n) (a^(2^k) + y^(2^k)) of the same quotient"""
    out = 1
    for _ in range(lg_n):
        out = out * (a + y) % r
        a, y = a * a % r, y * y % r
    return out


def coset_scale(p, g, n, r):
    """coefficients of p(g X), zero-padded to n"""
    out, pw = [], 1
    for j in range(n):
        out.append(p[j] * pw % r if j < len(p) else 0)
        pw = pw * g % r
    return out


def ntt_by_definition(a, w, r):
    """out[i] = sum_j a_j w^(i j)"""
    n = len(a)
    return [sum(a[j] * pow(w, i * j % n, r) for j in range(n)) % r for i in range(n)]


# ---- the pointwise formulas, as the comments of csrc/gpu.hpp state them
def q1_coset_pointwise(rr, za, zb, t, z, ca, cb, cz, eta_a, eta_b, eta_c, r):
    """out[i] = r[i] (eta_a A + eta_b B + eta_c A B) - t[i] Z  with A = za[i] + ca, B = zb[i] + cb, Z = z[i] + cz"""
    out = []
    for i in range(len(rr)):
        A, B, Z = za[i] + ca, zb[i] + cb, z[i] + cz
        out.append((rr[i] * (eta_a * A + eta_b * B + eta_c * A * B) - t[i] * Z) % r)
    return out


def h2_coset(row, col, va, vb, vc, rc, f, alpha, beta, alpha_beta, ea, eb, ec, vinv, r):
    """out = ((ea va + eb vb + ec vc) - (alpha beta - alpha row - beta col + row_col) f) * vinv"""
    out = []
    for i in range(len(row)):
        a = ea * va[i] + eb * vb[i] + ec * vc[i]
        b = alpha_beta - alpha * row[i] - beta * col[i] + rc[i]
        out.append((a - b * f[i]) * vinv % r)
    return out


def q1_combine(q0, q1, q3, mask, inv2, inv2zeta, r):
    """q = q_lo + X^n q_mid + X^2n q_hi has Q0 = q_lo + q_mid + q_hi on H, Q1 = q_lo + zeta q_mid - q_hi on W H, Q3 = q_lo - zeta q_mid - q_hi on W^3 H.  The quotient of
    q + mask by X^n - 1 is (q_mid + q_hi + m_mid + m_hi) + X^n (q_hi + m_hi), the remainder Q0 + m_lo + m_mid + m_hi; g_1 is the remainder without its constant term."""
    n = len(q0)
    h1, g1 = [0] * (2 * n), [0] * max(n - 1, 0)
    for i in range(n):
        q_mid = (q1[i] - q3[i]) * inv2zeta % r                       # Q1 - Q3 = 2 zeta q_mid
        q_hi = ((q0[i] - q_mid) - (q1[i] + q3[i]) * inv2) * inv2 % r   # Q0 - q_mid = q_lo + q_hi,  (Q1 + Q3) / 2 = q_lo - q_hi
        h1[i] = (q_mid + q_hi + mask[n + i] + mask[2 * n + i]) % r
        h1[n + i] = (q_hi + mask[2 * n + i]) % r
        if i >= 1:
            g1[i - 1] = (q0[i] + mask[i] + mask[n + i] + mask[2 * n + i]) % r
    return h1, g1


def z_poly_from_w(w, x, n, r):
    """w (X^m - 1) + x with m = len(x): n + 1 coefficients"""
    m, out = len(x), []
    for i in range(n + 1):
        v = 0
        if i >= m and i - m < len(w):
            v += w[i - m]
        if i < len(w):
            v -= w[i]
        if i < m:
            v += x[i]
        out.append(v % r)
    return out
