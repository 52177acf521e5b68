"""A structural determinism audit of an R1CS, and the same propagation run over values as a witness solver.

Input: the CSR triples (rowptr, col, coeff) of A, B and C, as api.circuit_matrix and api.circuit_matrix_gcm_segment return them, and a set of variables declared
known.  Row i says (A_i . z) (B_i . z) = C_i . z over the scalar field of BLS12-377 (r = r1cs_model.R377); variable 0 is One.  The audit answers: which variables do
the rows pin to ONE value once the known ones are fixed?  A variable it leaves over is one a prover may be free to choose -- an under-constrained circuit -- or one
whose determination needs a rule this module does not have.  Nothing here looks at a witness: the audit is about every assignment that satisfies the rows.

Booleanity.  u is marked boolean when some row has an empty C and A = a0 + a1 u, B = b0 + b1 u over One and u alone, a1 and b1 non-zero, with the roots -a0 / a1 and
-b0 / b1 being 0 and 1 (in either order).  The field has no zero divisors, so the row holds iff u is a root of one factor: u is 0 or 1 in every satisfying assignment.

Propagation.  A worklist runs over the rows.  A row is looked at when all its unknowns sit on one linear side:
  the C side, with every variable of A and B known: then (A . z) (B . z) is a known value t and the row reads  sum of the unknown terms of C = t - known terms;
  the A side (or B), when the other factor is k One with k != 0 and nothing else and C is fully known: then A . z = (C . z) / k, again linear in the unknowns.
Nothing value dependent counts: an unknown in a factor whose co-factor holds a variable is never determined from that row, even if the co-factor is fully known (it may
be zero on some assignment, and then the row says nothing about the unknown).  In that linear equation  sum_i c_i x_i = t  one of two rules must hold:
  R1: exactly one unknown, c != 0.  x = t / c: the field is a field, the solution exists and is unique.
  R2: several unknowns, every one marked boolean, the c_i distinct powers of two 2^(e_i) of one sign, and their sum below r.  Every x_i is 0 or 1 in every satisfying
      assignment (its booleanity row), so s = sum_i 2^(e_i) x_i is an INTEGER in [0, sum 2^(e_i)] < r; two such integers that agree mod r are equal, and an integer has one
      representation as a sum of distinct powers of two.  So the residue +-t fixes every x_i -- and if it is no such sum, no assignment satisfies the row.
Both rules are monotone (a row that determines its unknowns still does when fewer of them are unknown), so the set of determined variables does not depend on the order
the worklist takes.  What the rules refuse, each with the satisfying pair of assignments that shows why: a repeated weight (x1 + x2 = 1 has (1, 0) and (0, 1)); a member
without a booleanity row (x1 + 2 x2 = 2 has (0, 1) and (2, 0)); mixed signs (x1 - x2 = 0 has (0, 0) and (1, 1)); an unknown under a non-constant factor (x b = 0 with
b = 0 leaves x free); a "booleanity" row with roots {0, 2}.  tests/test_r1cs_audit.py builds each of these and asserts the refusal.

Solver mode (values=...).  The same propagation over Python integers mod r: R1 solves its equation, R2 reads the bits of the residue and raises Unsolvable when the
residue is no sum of the row's weights.  The result is a full z computed from the matrices and the seeded values alone; every row is then checked, so rows that solved
nothing act as checks, and the first violated row is reported.
"""
import numpy as np

from r1cs_model import R377

R = R377
SAFE = 1 << 61                                                             # int64 products stay exact below this bound on |A z| |B z| and |C z|


class Unsolvable(Exception):
    """solver mode: a row has no solution under R2 (.row), or the determined assignment violates a row (.row = the first such row)"""

    def __init__(self, row, why):
        Exception.__init__(self, "row %d: %s" % (row, why))
        self.row = row


def csr(rows):
    """a CSR triple from a list of rows, each a dict {variable: coefficient}: the toy systems of the tests"""
    rowptr, col, coeff = [0], [], []
    for r in rows:
        for v in sorted(r):
            col.append(v)
            coeff.append(r[v])
        rowptr.append(len(col))
    return np.array(rowptr, dtype=np.uint32), np.array(col, dtype=np.uint32), np.array(coeff, dtype=np.int64)


def _canonical(rowptr, col, coeff, n_rows):
    """(rowptr, col, coeff) as int64 with every row sorted by variable, duplicates merged and zero coefficients dropped"""
    rowptr, col, coeff = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64), np.asarray(coeff, dtype=np.int64)
    assert len(rowptr) == n_rows + 1 and rowptr[0] == 0 and rowptr[-1] == len(col) == len(coeff) and np.all(np.diff(rowptr) >= 0)
    row = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(rowptr))
    if len(col) and not (np.all((np.diff(row) > 0) | (np.diff(col) > 0)) and np.all(coeff != 0)):
        order = np.lexsort((col, row))
        row, col, coeff = row[order], col[order], coeff[order]
        first = np.concatenate([[True], (np.diff(row) != 0) | (np.diff(col) != 0)])
        starts = np.nonzero(first)[0]
        coeff = np.add.reduceat(coeff, starts)
        row, col = row[starts], col[starts]
        keep = coeff != 0
        row, col, coeff = row[keep], col[keep], coeff[keep]
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n_rows))]).astype(np.int64)
    return rowptr, col, coeff, row


class System:
    """the three matrices of one R1CS, canonical, with what the propagation needs precomputed"""

    def __init__(self, mats, n_vars=None):
        assert len(mats) == 3
        self.n_rows = len(mats[0][0]) - 1
        self.rowptr, self.col, self.coeff, self.row = [], [], [], []
        for m in mats:
            rp, cl, co, rw = _canonical(m[0], m[1], m[2], self.n_rows)
            self.rowptr.append(rp), self.col.append(cl), self.coeff.append(co), self.row.append(rw)
        top = max([int(c.max()) + 1 for c in self.col if len(c)] + [1])
        self.n_vars = top if n_vars is None else int(n_vars)
        assert top <= self.n_vars
        self.count = [np.diff(rp) for rp in self.rowptr]
        # a factor that is k One, k != 0, and nothing else (canonical rows hold no zero coefficient, and |k| < 2^63 < r)
        self.constant = []
        for s in range(2):
            one = np.zeros(self.n_rows, dtype=bool)
            single = np.nonzero(self.count[s] == 1)[0]
            one[single] = self.col[s][self.rowptr[s][single]] == 0
            self.constant.append(one)
        self.occurs = np.zeros(self.n_vars, dtype=bool)
        for c in self.col:
            self.occurs[c] = True
        self.boolean, self.boolean_row = self._booleans()
        self._occ = None

    def without_rows(self, rows):
        """the system with these rows emptied (a deleted constraint: 0 * 0 = 0)"""
        drop = np.zeros(self.n_rows, dtype=bool)
        drop[list(rows)] = True
        mats = []
        for s in range(3):
            keep = ~drop[self.row[s]]
            rp = np.concatenate([[0], np.cumsum(np.bincount(self.row[s][keep], minlength=self.n_rows))])
            mats.append((rp, self.col[s][keep], self.coeff[s][keep]))
        return System(mats, self.n_vars)

    def with_entry(self, side, row, var, coeff):
        """the system with one more term in one row"""
        mats = []
        for s in range(3):
            rw, cl, co = self.row[s], self.col[s], self.coeff[s]
            if s == side:
                rw, cl, co = np.append(rw, row), np.append(cl, var), np.append(co, coeff)
                order = np.argsort(rw, kind="stable")
                rw, cl, co = rw[order], cl[order], co[order]
            mats.append((np.concatenate([[0], np.cumsum(np.bincount(rw, minlength=self.n_rows))]), cl, co))
        return System(mats, self.n_vars)

    def _affine(self, s, rows):
        """for these rows of side s: (ok, u, c0, c1) with the row = c0 One + c1 u, u != One"""
        n, lo = self.count[s][rows], self.rowptr[s][rows]
        ok = (n == 1) | (n == 2)
        lo = np.where(ok, lo, 0)
        pad = lambda a: np.concatenate([a, [0, 0]])
        col, coeff = pad(self.col[s]), pad(self.coeff[s])
        first, second = col[lo], col[lo + 1]
        two = n == 2
        ok &= np.where(two, (first == 0) & (second != 0), first != 0)         # canonical rows are sorted: One comes first
        u = np.where(two, second, first)
        c0 = np.where(two, coeff[lo], 0)
        c1 = np.where(two, coeff[lo + 1], coeff[lo])
        return ok, u, c0, c1

    def _booleans(self):
        rows = np.nonzero((self.count[2] == 0) & (self.count[0] >= 1) & (self.count[0] <= 2) & (self.count[1] >= 1) & (self.count[1] <= 2))[0]
        oka, ua, a0, a1 = self._affine(0, rows)
        okb, ub, b0, b1 = self._affine(1, rows)
        ok = oka & okb & (ua == ub)
        # roots {0, 1}: one factor vanishes at 0 (c0 = 0), the other at 1 (c0 = -c1); int64 equality is equality mod r
        ok &= ((a0 == 0) & (b0 == -b1)) | ((b0 == 0) & (a0 == -a1))
        boolean = np.zeros(self.n_vars, dtype=bool)
        where = np.full(self.n_vars, -1, dtype=np.int64)
        boolean[ua[ok]] = True
        where[ua[ok][::-1]] = rows[ok][::-1]                                  # the first such row of each variable
        return boolean, where

    def occurrences(self):
        """(ptr, code, coeff): the entries of variable v are [ptr[v], ptr[v + 1]), each with code = 4 row + side and its coefficient; Python lists"""
        if self._occ is None:
            col = np.concatenate(self.col)
            code = np.concatenate([4 * self.row[s] + s for s in range(3)])
            order = np.argsort(col, kind="stable")
            ptr = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=self.n_vars))])
            self._occ = (ptr.tolist(), code[order].tolist(), np.concatenate(self.coeff)[order].tolist())
        return self._occ

    def defining_rows(self, var, side=None):
        """the rows that hold `var` (on `side` only, if given)"""
        sides = range(3) if side is None else (side,)
        return sorted({int(r) for s in sides for r in self.row[s][self.col[s] == var]})

    # ---- values
    def side_sums(self, z64):
        """[A z, B z, C z] in wrapping int64 (exact for every row whose true sums fit)"""
        out = []
        for s in range(3):
            acc = np.concatenate([[0], np.cumsum(self.coeff[s] * z64[self.col[s]])])
            out.append(acc[self.rowptr[s][1:]] - acc[self.rowptr[s][:-1]])
        return out

    def safe_rows(self, zmax):
        """the rows on which |A z| |B z| and |C z| stay below 2^61 for every z with |z_i| <= zmax: int64 is exact there (the bounds are sums of |coefficient| in
        float64, whose rounding is far inside the factor 4 between 2^61 and int64's range)"""
        b = []
        for s in range(3):
            acc = np.concatenate([[0.0], np.cumsum(np.abs(self.coeff[s]).astype(np.float64))])
            b.append((acc[self.rowptr[s][1:]] - acc[self.rowptr[s][:-1]]) * float(zmax))
        return (b[0] * b[1] < SAFE) & (b[2] < SAFE) & (b[0] < SAFE) & (b[1] < SAFE)

    def row_values(self, row, z):
        """(A z, B z, C z) of one row in Python integers mod r; z indexable by variable"""
        out = []
        for s in range(3):
            lo, hi = int(self.rowptr[s][row]), int(self.rowptr[s][row + 1])
            out.append(sum(k * int(z[v]) for v, k in zip(self.col[s][lo:hi].tolist(), self.coeff[s][lo:hi].tolist())) % R)
        return out

    def unsatisfied(self, z):
        """(rows where (A z)(B z) != C z mod r, how many rows went through int64, how many through Python integers); z = integers mod r, one per variable"""
        zc = [v if v <= R // 2 else v - R for v in (int(x) % R for x in z)]
        zmax = max(1, max(abs(v) for v in zc))
        if zmax < 1 << 31:
            z64 = np.array(zc, dtype=np.int64)
            safe = self.safe_rows(zmax)
            sa, sb, sc = self.side_sums(z64)
            bad = np.nonzero(safe & (sa * sb != sc))[0].tolist()
        else:
            safe, bad = np.zeros(self.n_rows, dtype=bool), []
        slow = np.nonzero(~safe)[0].tolist()
        for row in slow:
            a, b, c = self.row_values(row, zc)
            if (a * b - c) % R:
                bad.append(row)
        return sorted(bad), int(safe.sum()), len(slow)


class Result:
    def __init__(self, system, known, free, used, z):
        self.known, self.free, self.used_rows, self.z = known, free, used, z
        self.undetermined = np.nonzero(system.occurs & ~known)[0]             # variables no row holds are reported by dangling(), not here


def propagate(system, seed, values=None, greedy=None):
    """the audit (values None) or the solver (values = {variable: value} for every seeded variable).

    seed: the variables declared known.  greedy = an iterable of variables in the order to try: whenever the worklist runs dry, the first of them that is still
    undetermined is declared free (and known) and the propagation goes on; Result.free lists them.  Returns a Result: .known (bool per variable), .undetermined,
    .free, .used_rows (the rows that determined something) and, in solver mode, .z (a list of integers mod r, None where undetermined).

    Per row and side (slot 4 row + side) the loop keeps the number of unknown entries, the sum of their variables and the sum of their coefficients -- with one
    unknown left these ARE the variable and its coefficient, so R1 never scans a row -- the number of unknown entries that are not marked boolean, so that only a
    row R2 may accept is scanned, and, in solver mode, the value of the known part."""
    ptr, code, coef = system.occurrences()
    n4 = 4 * system.n_rows
    cnt, sumv, sumk, loose = [0] * n4, [0] * n4, [0] * n4, [0] * n4            # loose = the unknown entries whose variable is not marked boolean: R2 needs none
    for s in range(3):
        cnt[s:n4:4] = system.count[s].tolist()
        for into, what in ((sumv, system.col[s]), (sumk, system.coeff[s]), (loose, ~system.boolean[system.col[s]])):
            acc = np.concatenate([[0], np.cumsum(what)])
            into[s:n4:4] = (acc[system.rowptr[s][1:]] - acc[system.rowptr[s][:-1]]).tolist()
    const = [False] * n4
    const[0:n4:4], const[1:n4:4] = system.constant[0].tolist(), system.constant[1].tolist()
    rowptr, col, coeff = system.rowptr, system.col, system.coeff
    boolean = system.boolean.tolist()
    known = bytearray(system.n_vars)
    solving = values is not None
    z = [None] * system.n_vars if solving else None
    part = [0] * n4 if solving else None                                     # the known part of (side . z)
    stack, used, free = [], [], []

    def rhs(base, side, have):
        """the value the unknown terms of this side add up to; have = the side's known part"""
        if side == 2:
            return part[base] * part[base + 1] - have
        return part[base + 2] * pow(part[base + 1 - side], -1, R) - have

    def learn(u, value):
        known[u] = 1
        stack.append(u)
        if solving:
            z[u] = value % R

    def scan(base, side):
        """the slow path, R2: several entries of the side count as unknown.  Some may be known already and wait on the stack (their terms are not in `part` yet), so
        the unknowns and the known part are read from the row itself"""
        row = base >> 2
        lo, hi = rowptr[side][row], rowptr[side][row + 1]
        ents = list(zip(col[side][lo:hi].tolist(), coeff[side][lo:hi].tolist()))
        unk = [(v, k) for v, k in ents if not known[v]]
        if not unk:
            return
        t = rhs(base, side, sum(k * z[v] for v, k in ents if known[v])) if solving else None
        if len(unk) == 1:
            used.append(row)
            v, k = unk[0]
            learn(v, None if t is None else t * pow(k, -1, R))
            return
        sign = 1 if unk[0][1] > 0 else -1
        weights = [sign * k for _, k in unk]
        if not all(boolean[v] for v, _ in unk) or any(w <= 0 or w & (w - 1) for w in weights) or len(set(weights)) != len(weights) or sum(weights) >= R:
            return
        used.append(row)
        if solving:
            t = sign * t % R
            if t > sum(weights) or t & ~sum(weights):
                raise Unsolvable(row, "the residue %d is no sum of the weights %s" % (t, sorted(weights)))
        for (v, _), w in zip(unk, weights):
            learn(v, int(bool(t & w)) if solving else None)

    for v in seed:
        if not known[v]:
            known[v] = 1
            stack.append(v)
            if solving:
                z[v] = values[v] % R
    assert not solving or z[0] == 1, "One is seeded with 1"
    order = iter(greedy) if greedy is not None else None
    while True:
        while stack:
            v = stack.pop()
            zv = z[v] if solving else 0
            lv = 0 if boolean[v] else 1
            for i in range(ptr[v], ptr[v + 1]):
                c, k = code[i], coef[i]
                cnt[c] -= 1
                loose[c] -= lv
                sumv[c] -= v
                sumk[c] -= k
                if solving:
                    part[c] += k * zv
                base = c & -4
                if cnt[base] == 0:
                    if cnt[base + 1] == 0:
                        side = 2
                    elif cnt[base + 2] == 0 and const[base]:
                        side = 1
                    else:
                        continue
                elif cnt[base + 1] == 0 and cnt[base + 2] == 0 and const[base + 1]:
                    side = 0
                else:
                    continue
                n = cnt[base + side]
                if n == 1:                                                   # R1: canonical rows hold no zero coefficient
                    u = sumv[base + side]
                    if known[u]:                                             # determined already and waiting on the stack: its entries are still counted
                        continue
                    known[u] = 1
                    stack.append(u)
                    used.append(base >> 2)
                    if solving:
                        k = sumk[base + side]
                        z[u] = rhs(base, side, part[base + side]) * (k if k == 1 or k == -1 else pow(k, -1, R)) % R
                elif n > 1 and not loose[base + side]:
                    scan(base, side)
        if order is None:
            break
        nxt = next((v for v in order if not known[v]), None)
        if nxt is None:
            break
        free.append(nxt)
        known[nxt] = 1
        stack.append(nxt)
    return Result(system, np.frombuffer(bytes(known), dtype=np.uint8).astype(bool), free, used, z)


def solve(system, values):
    """a full z (list of integers mod r) from the seeded values alone; raises Unsolvable with the first row the determined assignment violates, or when a variable
    that occurs in a row stays undetermined (.row = -1).  Variables that no row holds come back as 0"""
    res = propagate(system, sorted(values), values=values)
    if len(res.undetermined):
        raise Unsolvable(-1, "%d variables are not determined, the first %s" % (len(res.undetermined), res.undetermined[:8].tolist()))
    z = [0 if v is None else v for v in res.z]
    bad, _, _ = system.unsatisfied(z)
    if bad:
        raise Unsolvable(bad[0], "violated by the determined assignment")
    return z, res


def dangling(system, real):
    """(real variables that no row holds, other variables that a row holds); real = a bool per variable"""
    real = np.asarray(real, dtype=bool)
    return np.nonzero(real & ~system.occurs)[0], np.nonzero(~real & system.occurs)[0]


def unperturbable(system, z, replacements):
    """exhaustive single-variable perturbation of a satisfying z (small integers, one per variable).  replacements: {name: function of the int64 array z giving the
    replacement of every variable}.  For every variable that occurs in a row and every replacement, only the rows that hold the variable are recomputed:
    A z + a d, B z + b d, C z + c d with d = the change and a, b, c the variable's coefficients in that row.  Returns ({name: variables whose replacement left every
    row satisfied}, {"pairs", "int64", "python"}: how many (variable, row) pairs there are and which arithmetic each went through)"""
    z64 = np.asarray(z, dtype=np.int64)
    n = system.n_rows
    key = np.concatenate([system.col[s] * n + system.row[s] for s in range(3)])
    uniq, inv = np.unique(key, return_inverse=True)
    pv, pr = uniq // n, uniq % n
    c = np.zeros((3, len(uniq)), dtype=np.int64)
    at = 0
    for s in range(3):
        c[s, inv[at:at + len(system.col[s])]] = system.coeff[s]
        at += len(system.col[s])
    sums = system.side_sums(z64)
    assert not np.any(system.safe_rows(int(np.abs(z64).max())) & (sums[0] * sums[1] != sums[2])), "z does not satisfy the system"
    out, paths = {}, {"pairs": len(uniq), "int64": 0, "python": 0}
    for name, fn in replacements.items():
        new = np.asarray(fn(z64), dtype=np.int64)
        d = (new - z64)[pv]
        assert np.all(d != 0), "a replacement that changes nothing"
        safe = system.safe_rows(max(int(np.abs(z64).max()), int(np.abs(new).max())))[pr]
        na, nb, nc = (sums[s][pr] + c[s] * d for s in range(3))
        broken = np.zeros(system.n_vars, dtype=bool)
        broken[pv[safe & (na * nb != nc)]] = True
        slow = np.nonzero(~safe)[0]
        for i in slow.tolist():
            v, row = int(pv[i]), int(pr[i])
            zz = {v: int(new[v])}
            a, b, cc = system.row_values(row, _Patched(z64, zz))
            if (a * b - cc) % R:
                broken[v] = True
        paths["int64"], paths["python"] = int(safe.sum()), len(slow)
        assert paths["int64"] + paths["python"] == paths["pairs"]
        out[name] = np.nonzero(system.occurs & ~broken)[0]
    return out, paths


class _Patched:
    def __init__(self, base, patch):
        self.base, self.patch = base, patch

    def __getitem__(self, v):
        return self.patch[v] if v in self.patch else int(self.base[v])
