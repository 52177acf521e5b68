"""A plain model of what the key-synthesis kernels compute, on Python integers over tools/curve_math.py: powers and scalar multiples of a base (csrc/kernels_msm.hip
k_power_scalars, k_fixed_base), a window-table copy (k_table_next), the Niels triple of a Weierstrass point (k_convert_bases_te) and the values of the six index
polynomials on K (csrc/kernels_poly.hip k_index_rowcol, k_index_vals; ark-marlin's arithmetize_matrix).  Nothing here shares structure with the kernels: double-and-add
instead of byte windows, one inversion per point instead of shared ones, one entry at a time.  tests/test_keysynth_model.py pins it against the CPU oracle;
tests/test_gpu_keysynth.py compares the kernels with it and with the oracle.

A point is an affine pair of integers or None for infinity; scalars and field elements are canonical integers."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools import curve_math as cm                     # noqa: E402
import msm_model                                       # noqa: E402
import r1cs_model                                      # noqa: E402

FR = {377: cm.R377, 381: cm.R381}
FQ = {377: cm.Q377, 381: cm.Q381}
GEN = {377: cm.G1_377, 381: cm.G1_381}
ORDER2_377 = (cm.Q377 - 1, 0)                          # (-1, 0) on y^2 = x^3 + 1: the point of order 2, which no subgroup point is
TE = cm.edwards_377()


# ---- points as the library's 96 bytes: x || y in Montgomery form (radix 2^384), infinity = 96 zero bytes
def pt_bytes(pt, cid=377):
    if pt is None:
        return bytes(96)
    q = FQ[cid]
    return b"".join((c % q * (1 << 384) % q).to_bytes(48, "little") for c in pt)


def pt_from_bytes(buf, cid=377):
    if buf == bytes(96):
        return None
    q = FQ[cid]
    ri = pow(1 << 384, -1, q)
    return tuple(int.from_bytes(buf[i:i + 48], "little") * ri % q for i in (0, 48))


def pts_bytes(pts, cid=377):
    return b"".join(pt_bytes(p, cid) for p in pts)


def mul(k, pt, cid=377):
    """k * pt, k reduced modulo the group order first (so that k = r gives infinity without a walk over a long scalar)"""
    return None if pt is None else cm.ec_mul(k % FR[cid], pt, FQ[cid])


# ---- fixed-base kernels
def powers(base, beta, start, count, cid=377):
    """[beta^(start + i) * base for i < count]; 0^0 = 1 as Fp::pow gives it"""
    r = FR[cid]
    return [mul(pow(beta, start + i, r), base, cid) for i in range(count)]


def power_scalars(beta, start, count, cid=377):
    return [pow(beta, start + i, FR[cid]) for i in range(count)]


def scalar_multiples(base, scalars, cid=377):
    return [mul(s, base, cid) for s in scalars]


# ---- window tables
def table_layout(c, cid=377):
    """(nwin, c_hi, n_hi) of TableLayout over the bits of r plus the recoding carry's"""
    return msm_model.table_layout(c, FR[cid].bit_length() + 1)


def table_offset(c, j, cid=377):
    """the bit offset of window j: copy j of the tables holds 2^offset(j) * P"""
    nwin, c_hi, n_hi = table_layout(c, cid)
    assert 0 <= j < nwin
    return j * c_hi if j < n_hi else n_hi * c_hi + (j - n_hi) * (c_hi - 1)


def table_width(c, j, cid=377):
    _, c_hi, n_hi = table_layout(c, cid)
    return c_hi if j < n_hi else c_hi - 1


def table_copy(pt, c, j, cid=377):
    """2^offset(j) * pt by plain doublings (any curve point: the order-2 point goes to infinity at the first one)"""
    for _ in range(table_offset(c, j, cid)):
        pt = cm.ec_add(pt, pt, FQ[cid])
    return pt


# ---- the Edwards form
def niels_triple(pt):
    """(y - x, y + x, 2 d x y) mod q of the point's image on the a = -1 twisted Edwards model; infinity -> the identity's (1, 1, 0)"""
    x, y = cm.te_from_weierstrass(pt, TE)
    q = cm.Q377
    return ((y - x) % q, (y + x) % q, TE["k2d"] * x * y % q)


# ---- the index polynomials on K
def joint_entries(mats):
    """per-row sorted union of the column supports of A, B, C (ark-marlin's sum_matrices) -> [(row, column, coeff_a, coeff_b, coeff_c)], absent coefficients 0"""
    rows = len(mats[0][0]) - 1
    out = []
    for r in range(rows):
        per = {}
        for q, (rowptr, col, coeff) in enumerate(mats):
            for i in range(int(rowptr[r]), int(rowptr[r + 1])):
                per.setdefault(int(col[i]), [0, 0, 0])[q] = int(coeff[i])
        out += [(r, c) + tuple(per[c]) for c in sorted(per)]
    return out


def index_inputs(mats, n, m):
    """what the key hands to index_evals: (ci = the column's position on H, ri, ca, cb, cc) per joint entry"""
    e = joint_entries(mats)
    return [r1cs_model.reindex(n, m, c) for _, c, _, _, _ in e], [r for r, _, _, _, _ in e], [a for _, _, a, _, _ in e], [b for _, _, _, b, _ in e], [c for _, _, _, _, c in e]


def index_values(ci, ri, ca, cb, cc, lg_k, lg_n, r=cm.R377):
    """arithmetize_matrix on the size-2^lg_n domain H: entry i at (row ri, column position ci) gives row = h^ci (the matrix is taken transposed), col = h^ri,
    row_col = their product and val_M = coeff_M / u_H(row, row) with u_H(x, x) = |H| x^(|H| - 1); the entries up to |K| are padded with row = col = row_col = 1, val = 0.
    Returns the six lists and 1 / u_H per entry (0 on the padding)."""
    n, k, g = 1 << lg_n, 1 << lg_k, r1cs_model.domain_gen(lg_n, r)
    assert len(ci) <= k
    out = {name: [] for name in ("row", "col", "row_col", "val_a", "val_b", "val_c", "u_inv")}
    for c, rw, a, b, cv in zip(ci, ri, ca, cb, cc):
        row, col = pow(g, c, r), pow(g, rw, r)
        u_inv = pow(n * pow(row, n - 1, r), -1, r)
        for name, v in (("row", row), ("col", col), ("row_col", row * col), ("val_a", a * u_inv), ("val_b", b * u_inv), ("val_c", cv * u_inv), ("u_inv", u_inv)):
            out[name].append(v % r)
    pad = k - len(ci)
    for name in out:
        out[name] += [1 if name in ("row", "col", "row_col") else 0] * pad
    return out
