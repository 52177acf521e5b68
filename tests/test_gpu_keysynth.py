"""GPU parity tests of the kernels that BUILD A KEY, each through a kernel-level C entry point (include/zkaes.h): the fixed-base kernels behind the universal SRS, both
Lagrange-basis SRS arrays and the serialized powers (k_power_scalars, k_fixed_base), the window-table step (k_table_next), the Edwards conversion (k_convert_bases_te) and
the indexer (k_index_rowcol, batch_inverse over zeros, k_index_vals).  They run once per SRS or key; whole-key tests reach none of their edges.

References: points come from the CPU oracle (zko_api_g1_mul, zko_api_fixed_base, zko_api_msm) at scalars worked out here with Python integers; the Niels triples and the
index values come from tests/keysynth_model.py, which tests/test_keysynth_model.py pins against the oracle.  EVERY comparison is exact: bytes for affine points and field
elements, 96 zero bytes for the point at infinity, values mod q (plus te28.cuh's bound on a stored coordinate) for Niels records.  The oracle never sees an infinity base:
its loader does not read (0, 0) as one."""
import ctypes as C
import random

import numpy as np
import pytest

import arith_model as am
import keysynth_model as km
from test_keysynth_model import oracle_generator, oracle_mul, oracle_points

pytestmark = pytest.mark.gpu

INF = bytes(96)
CURVES = [377, 381]
B32, B40 = 1 << 32, 1 << 40
OTHER_BASE = 0x6B65797379              # the base that is not the generator: this multiple of it


def split96(buf):
    return [buf[i:i + 96] for i in range(0, len(buf), 96)]


def same_points(got, want, what):
    got = split96(got) if isinstance(got, (bytes, bytearray)) else list(got)
    assert len(got) == len(want), "%s: %d points, expected %d" % (what, len(got), len(want))
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, "%s: %d of %d points differ from the reference, first at index %d (%s)" % (
        what, len(bad), len(want), bad[0], "reference is infinity" if want[bad[0]] == INF else "got infinity" if got[bad[0]] == INF else "both finite")


class Ref:
    """the oracle's multiples of the two bases, remembered per scalar: many cases share 0, 1, r - 1 and the low powers"""

    def __init__(self, zko):
        self.zko, self.cache = zko, {}

    def base(self, cid, which):
        g = oracle_generator(self.zko, cid)
        return g if which == "generator" else oracle_mul(self.zko, cid, g, OTHER_BASE)

    def multiples(self, cid, which, scalars):
        r = self.zko.FR[cid]
        missing = sorted({k % r for k in scalars if (cid, which, k % r) not in self.cache})
        if which == "generator":
            pts = oracle_points(self.zko, cid, missing)
        else:
            b = self.base(cid, which)
            pts = [oracle_mul(self.zko, cid, b, k) if k else INF for k in missing]
        for k, p in zip(missing, pts):
            self.cache[(cid, which, k)] = p
        return [self.cache[(cid, which, k % r)] for k in scalars]

    def subgroup_points(self, cid, n, seed):
        rnd = random.Random(seed)
        return oracle_points(self.zko, cid, [rnd.randrange(1, self.zko.FR[cid]) for _ in range(n)])

    def doubled(self, cid, pts, bits):
        """2^bits * P per point; infinity stays, BLS12-377's order-2 point goes to infinity (the oracle is asked for subgroup points only)"""
        if bits == 0:
            return list(pts)
        order2 = km.pt_bytes(km.ORDER2_377) if cid == 377 else None
        return [INF if p in (INF, order2) else oracle_mul(self.zko, cid, p, 1 << bits) for p in pts]


@pytest.fixture(scope="module")
def ref(zko):
    return Ref(zko)


# ---- fixed_base_powers -----------------------------------------------------------------------------------------------------------------------------------------------------
BETAS = ["zero", "one", "minus one", "two", "random"]
STARTS = [0, 1, B32 - 3, B40 + 5]


def beta_value(name, cid):
    r = km.FR[cid]
    return {"zero": 0, "one": 1, "minus one": r - 1, "two": 2, "random": random.Random(cid * 31).randrange(2, r - 1)}[name]


def power_cases(bi):
    """(count, start) for beta number bi: every start with every beta; the counts 1, 63, 64, 65 rotate over them, and the start three below 2^32 always gets at least 63
    outputs, so that exponents sit on both sides of the 32-bit boundary"""
    out = []
    for fi, start in enumerate(STARTS):
        out.append(([63, 64, 65][bi % 3] if start == B32 - 3 else [1, 63, 64, 65][(fi + bi) % 4], start))
    return out


def test_the_power_cases_cover_every_count_start_and_beta():
    seen = [c for bi in range(len(BETAS)) for c in power_cases(bi)]
    assert {c for c, _ in seen} == {1, 63, 64, 65} and {s for _, s in seen} == set(STARTS)
    assert all(c >= 6 for c, s in seen if s == B32 - 3)


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("base", ["generator", "other"])
@pytest.mark.parametrize("cid", CURVES)
def test_fixed_base_powers_equal_the_oracles_multiples(ref, zko, api, cid, base, beta):
    b, base_xy = beta_value(beta, cid), ref.base(cid, base)
    for count, start in power_cases(BETAS.index(beta)):
        scalars = km.power_scalars(b, start, count, cid)
        got = api.fixed_base_powers(cid, base_xy, zko.fr_pack([b], cid), start, count)
        same_points(got, ref.multiples(cid, base, scalars), "beta = %s, from = %d, count = %d" % (beta, start, count))
        if beta == "zero":
            assert split96(got) == ([base_xy] if start == 0 else [INF]) + [INF] * (count - 1), "0^0 = 1 gives the base, every other power of zero infinity"


@pytest.mark.parametrize("base", ["generator", "other"])
@pytest.mark.parametrize("cid", CURVES)
def test_fixed_base_powers_do_not_depend_on_the_chunk(ref, zko, api, cid, base):
    """300 points from 100 below 2^32 in chunks of 64, 97, 300 and the default: the chunk loop's `from + off` and `out + off` run more than once, and the 32-bit boundary
    falls inside the second chunk of 64 and of 97"""
    b, base_xy, start, count = beta_value("random", cid), ref.base(cid, base), B32 - 100, 300
    want = ref.multiples(cid, base, km.power_scalars(b, start, count, cid))
    got = {chunk: api.fixed_base_powers(cid, base_xy, zko.fr_pack([b], cid), start, count, chunk=chunk) for chunk in (64, 97, 300, 0)}
    for chunk, pts in got.items():
        same_points(pts, want, "chunk = %d" % chunk)
    assert len(set(got.values())) == 1


# ---- fixed_base_scalars ----------------------------------------------------------------------------------------------------------------------------------------------------
def edge_scalars_130():
    """130 scalars of BLS12-377: zeros at lanes 0, 63 and 64 (the last lane of a wave and the first of the next), 1, r - 1, a single 1 and a single 255 in every byte window
    that stays below r, two scalars whose every other byte is zero, and random ones"""
    r, rnd = km.FR[377], random.Random("fixed base scalars")
    body = [1, r - 1] + [1 << (8 * w) for w in range(32) if 1 << (8 * w) < r] + [255 << (8 * w) for w in range(32) if 255 << (8 * w) < r]
    body += [sum(0xA5 << (16 * i) for i in range(16)), sum(0x5A << (16 * i + 8) for i in range(15)) | 0x0B << 248]
    assert all(0 < s < r for s in body) and len(body) == 2 + 32 + 31 + 2
    body += [rnd.randrange(1, r) for _ in range(127 - len(body))]
    out = [0] + body[:62] + [0, 0] + body[62:]
    assert len(out) == 130 and [i for i, s in enumerate(out) if s == 0] == [0, 63, 64]
    return out


@pytest.mark.parametrize("chunk", [0, 64])
@pytest.mark.parametrize("base", ["generator", "other"])
def test_fixed_base_scalars_equal_the_oracles_multiples(ref, zko, api, base, chunk):
    scalars = edge_scalars_130()
    got = api.fixed_base_scalars(ref.base(377, base), zko.fr_pack(scalars), chunk=chunk)
    same_points(got, ref.multiples(377, base, scalars), "130 edge scalars, chunk = %d" % chunk)
    assert [i for i, p in enumerate(split96(got)) if p == INF] == [0, 63, 64]


def test_fixed_base_scalars_of_a_lone_zero_and_of_all_zeros(ref, zko, api):
    """what acquire_lagrange feeds through on X: scalar 0 -> XYZZ infinity -> the all-zero affine point"""
    g = ref.base(377, "generator")
    assert api.fixed_base_scalars(g, zko.fr_pack([0])) == INF
    assert api.fixed_base_scalars(g, zko.fr_pack([0] * 65), chunk=64) == INF * 65


# ---- table_next / build_window_tables --------------------------------------------------------------------------------------------------------------------------------------
def nine_points(ref, cid):
    """one full batch of eight and a ragged batch of one: infinity at slot 2, the order-2 point (BLS12-377) or another infinity at slot 5"""
    pts = ref.subgroup_points(cid, 9, 900 + cid)
    pts[2] = INF
    pts[5] = km.pt_bytes(km.ORDER2_377) if cid == 377 else INF
    return pts


@pytest.fixture(scope="module")
def table_refs(ref):
    """(curve, window bits) -> the reference copies of nine_points: copy j = 2^offset(j) mod r times each point, by the oracle"""
    memo = {}

    def get(cid, c):
        if (cid, c) not in memo:
            pts = nine_points(ref, cid)
            memo[(cid, c)] = [ref.doubled(cid, pts, km.table_offset(c, j, cid)) for j in range(km.table_layout(c, cid)[0])]
        return memo[(cid, c)]
    return get


def table_js(c, cid):
    nwin, _, n_hi = km.table_layout(c, cid)
    return list(range(1, nwin)) if c == 13 else sorted({1, n_hi, n_hi + 1, nwin - 1})


@pytest.mark.parametrize("c", [13, 20])
@pytest.mark.parametrize("cid", CURVES)
def test_table_next_gives_copy_j_from_copy_j_minus_one(table_refs, api, cid, c):
    """every copy of the 13-bit plan, and the first copy, both sides of the width boundary n_hi and the last copy of the 20-bit plan: copies up to n_hi double c_hi times,
    the later ones c_hi - 1"""
    copies = table_refs(cid, c)
    nwin, c_hi, n_hi = km.table_layout(c, cid)
    assert 1 < n_hi < nwin - 1 and api.table_windows(cid, c) == nwin
    for j in table_js(c, cid):
        assert km.table_offset(c, j, cid) - km.table_offset(c, j - 1, cid) == (c_hi if j - 1 < n_hi else c_hi - 1)
        same_points(api.table_next(cid, b"".join(copies[j - 1]), c, j), copies[j], "copy %d of %d under %d bits" % (j, nwin, c))


@pytest.mark.parametrize("c", [13, 20])
@pytest.mark.parametrize("cid", CURVES)
def test_build_window_tables_equals_the_chain_of_steps_and_the_oracle(table_refs, ref, api, cid, c):
    pts = nine_points(ref, cid)
    nwin = km.table_layout(c, cid)[0]
    got = api.build_window_tables(cid, b"".join(pts), c)
    assert len(got) == 96 * 9 * nwin
    chain = [b"".join(pts)]
    for j in range(1, nwin):
        chain.append(api.table_next(cid, chain[-1], c, j))
    assert got == b"".join(chain), "build_window_tables differs from its own steps"
    same_points(got, [p for copy in table_refs(cid, c) for p in copy], "all %d copies under %d bits" % (nwin, c))


@pytest.mark.parametrize("count", [1, 7, 8, 9, 64 * 8 + 3])
@pytest.mark.parametrize("cid", CURVES)
def test_table_next_at_the_batch_and_wave_boundaries(ref, api, cid, count):
    """eight points per lane share one inversion: a lone point, a batch short of one, a full batch, one more, and 64 full lanes plus a ragged batch in a second wave"""
    pts = ref.subgroup_points(cid, count, 77 * count + cid)
    same_points(api.table_next(cid, b"".join(pts), 13, 1), ref.doubled(cid, pts, km.table_width(13, 0, cid)), "%d points" % count)


def infinity_arrangement(ref, cid, seed):
    """35 points = four batches of eight and a ragged one of three: infinity at the first, a middle and the last slot of a batch, a whole batch of infinities, and the ragged
    last batch holding nothing else"""
    pts = ref.subgroup_points(cid, 35, seed)
    for i in [0, 8 + 3, 16 + 7] + list(range(24, 32)) + [32, 33, 34]:
        pts[i] = INF
    return pts


@pytest.mark.parametrize("cid", CURVES)
def test_table_next_keeps_infinity_and_its_neighbours(ref, api, cid):
    """an infinity point takes the skip path of both loops; the shared inversion must not be poisoned for the other points of its batch"""
    pts = infinity_arrangement(ref, cid, 3500 + cid)
    n_hi = km.table_layout(13, cid)[2]
    for j in (1, n_hi + 1):
        got = api.table_next(cid, b"".join(pts), 13, j)
        same_points(got, ref.doubled(cid, pts, km.table_width(13, j - 1, cid)), "copy %d" % j)
        assert [i for i, p in enumerate(split96(got)) if p == INF] == [i for i, p in enumerate(pts) if p == INF]


def test_table_next_takes_the_order_two_point_to_infinity(ref, api):
    """(-1, 0) on y^2 = x^3 + 1: finite going in, infinity after the first doubling -- the skip is decided AFTER the doublings, and the batch's other points must be right"""
    pts = ref.subgroup_points(377, 9, 4242)
    pts[4], pts[6] = km.pt_bytes(km.ORDER2_377), INF
    got = api.table_next(377, b"".join(pts), 13, 1)
    same_points(got, ref.doubled(377, pts, 13), "order-2 point at slot 4")
    assert split96(got)[4] == INF


# ---- convert_bases_te ------------------------------------------------------------------------------------------------------------------------------------------------------
def check_niels(records, pts, what):
    """every record equals the model's triple as values mod q and keeps te28.cuh's form of a stored coordinate: normalized 28-bit limbs of a product (below 1.2 q)"""
    assert len(records) == len(pts)
    for i, (rec, p) in enumerate(zip(records, pts)):
        assert tuple(am.G377.unmont(c) for c in rec) == km.niels_triple(km.pt_from_bytes(p)), "%s: record %d differs from the model%s" % (what, i, " (an infinity point)" if p == INF else "")
        am._te_outputs_ok([sum(rec, [])], ncoord=3)
        assert all(x <= am.G377.mask for c in rec for x in c), "%s: record %d has a limb above 28 bits" % (what, i)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 64 * 8 + 5])
def test_convert_bases_te_equals_the_models_niels_triples(ref, api, n):
    pts = ref.subgroup_points(377, n, 5000 + n)
    check_niels(api.convert_bases_te(b"".join(pts)), pts, "%d points" % n)


def test_convert_bases_te_writes_the_identity_for_infinity_and_keeps_the_neighbours(ref, api):
    pts = infinity_arrangement(ref, 377, 5377)
    recs = api.convert_bases_te(b"".join(pts))
    check_niels(recs, pts, "infinities among 35 points")
    for i, p in enumerate(pts):
        if p == INF:
            assert tuple(am.G377.unmont(c) for c in recs[i]) == (1, 1, 0), "slot %d: an infinity point must give the Edwards identity" % i
    lone = api.convert_bases_te(INF)
    assert tuple(am.G377.unmont(c) for c in lone[0]) == (1, 1, 0)


def test_convert_bases_te_refuses_a_point_of_order_two(ref, api):
    pts = ref.subgroup_points(377, 9, 5999)
    pts[4] = km.pt_bytes(km.ORDER2_377)
    with pytest.raises(api.ZkAesError, match="order 2 or 4"):
        api.convert_bases_te(b"".join(pts))
    check_niels(api.convert_bases_te(b"".join(pts[:4] + pts[5:])), pts[:4] + pts[5:], "the good path after the refusal")


# ---- infinity bases through the consumers ----------------------------------------------------------------------------------------------------------------------------------
def oracle_msm(zko, pts, scalars):
    """sum of scalars[i] * pts[i] over the finite points with a non-zero scalar -> 96 bytes, infinity as zeros"""
    r = zko.FR[377]
    items = [(p, s % r) for p, s in zip(pts, scalars) if p != INF and s % r]
    if not items:
        return INF
    out = C.create_string_buffer(96)
    inf = zko.lib().zko_api_msm(377, b"".join(p for p, _ in items), zko.fr_pack([s for _, s in items]), C.c_size_t(len(items)), out)
    return INF if inf else out.raw


def bases_with_infinities(ref, n):
    pts = ref.subgroup_points(377, n, 8000 + n)
    holes = sorted({0, 15, 16, n - 1} | (set(range(32, 48)) | set(random.Random(n).sample(range(n), 60)) if n >= 1000 else {7}))
    for i in holes:
        pts[i] = INF
    return pts, holes


@pytest.mark.parametrize("srs", [True, False], ids=["edwards", "weierstrass"])
@pytest.mark.parametrize("c", [13, 20])
@pytest.mark.parametrize("n", [33, 1000])
def test_the_table_msm_takes_infinity_bases_under_non_zero_scalars(ref, zko, api, n, c, srs):
    """what a Lagrange-basis SRS holds on X: the all-zero affine point, whose window-table copies stay infinity and whose Niels record is the identity"""
    pts, holes = bases_with_infinities(ref, n)
    rnd = random.Random(n + c)
    scalars = [rnd.randrange(1, km.FR[377]) for _ in range(n)]
    scalars[holes[0]], scalars[holes[1]] = 1, km.FR[377] - 1
    xy, inf = api.msm_table(377, b"".join(pts), zko.fr_pack(scalars), c, srs=srs)
    want = oracle_msm(zko, pts, scalars)
    assert (INF if inf else xy) == want and want != INF


@pytest.mark.parametrize("edwards", [True, False], ids=["edwards", "weierstrass"])
@pytest.mark.parametrize("n", [33, 1000])
def test_the_class_sums_take_identity_bases_under_every_value(ref, zko, api, n, edwards):
    pts, holes = bases_with_infinities(ref, n)
    rs = np.random.RandomState(n)
    vecs = [rs.choice(np.array([0, 1, -1, 2, -2], dtype=np.int8), size=n) for _ in range(2)]
    for k, v in enumerate((1, -1, 2, -2)):                       # every value on an identity base, in both vectors
        vecs[0][holes[k]], vecs[1][holes[(k + 1) % 4]] = v, v
    vecs.append(np.where(np.isin(np.arange(n), holes), 2, 0).astype(np.int8))              # non-zero values on identity bases ONLY: the sum is infinity
    got = api.class_sum(b"".join(pts), vecs, edwards=edwards)
    for k, ((ok, xy, inf), v) in enumerate(zip(got, vecs)):
        assert ok, "class_sum declined vector %d: nothing in it is out of range" % k
        assert (INF if inf else xy) == oracle_msm(zko, pts, [int(x) for x in v]), "vector %d" % k
    assert got[2][2], "values on identity bases only must sum to infinity"


# ---- index_evals -----------------------------------------------------------------------------------------------------------------------------------------------------------
COEFFS = [(1, 0, 0), (0, -1, 0), (0, 0, 1 << 31), (-(1 << 62), 1, 0), (0, 1 << 31, -1), (1, -1, -(1 << 62)), (1 << 31, 0, -(1 << 62)), (-1, -(1 << 62), 1 << 31)]


def index_case(cnt, lg_n, seed):
    """cnt entries: the corners (0, n - 1), (n - 1, 0), (0, 0), (n - 1, n - 1) first, then random positions; the coefficient patterns rotate"""
    n, rnd = 1 << lg_n, random.Random(seed)
    corners = [(0, n - 1), (n - 1, 0), (0, 0), (n - 1, n - 1)]
    pos = (corners + [(rnd.randrange(n), rnd.randrange(n)) for _ in range(cnt)])[:cnt]
    co = [COEFFS[(i + seed) % len(COEFFS)] for i in range(cnt)]
    return [c for c, _ in pos], [r for _, r in pos], [a for a, _, _ in co], [b for _, b, _ in co], [c for _, _, c in co]


@pytest.mark.parametrize("which", ["none", "one", "k - 1", "k"])
@pytest.mark.parametrize("lg_k", [4, 9])
@pytest.mark.parametrize("lg_n", [3, 10])
def test_index_evals_equal_the_model(zko, api, lg_n, lg_k, which):
    k = 1 << lg_k
    cnt = {"none": 0, "one": 1, "k - 1": k - 1, "k": k}[which]
    ci, ri, ca, cb, cc = index_case(cnt, lg_n, 10 * lg_n + lg_k)
    want = km.index_values(ci, ri, ca, cb, cc, lg_k, lg_n)
    got = api.index_evals(ci, ri, ca, cb, cc, lg_k, lg_n)
    for name in ("row", "col", "row_col", "val_a", "val_b", "val_c", "u_inv"):
        assert got[name] == zko.fr_pack(want[name]), "%s differs from the model (cnt = %d of %d, |H| = %d)" % (name, cnt, k, 1 << lg_n)
    one, zero = zko.fr_pack([1]), bytes(32)
    for name in ("row", "col", "row_col"):
        assert got[name][32 * cnt:] == one * (k - cnt), "padding of %s must be the domain's first element" % name
    for name in ("val_a", "val_b", "val_c", "u_inv"):
        assert got[name][32 * cnt:] == zero * (k - cnt), "padding of %s must be zero" % name
    assert got["tails"] == b"\xab" * (7 * 32 * api.INDEX_EVALS_TAIL), "a kernel wrote behind the k outputs"


def test_index_evals_tell_the_row_from_the_column(zko, api):
    """one entry at column position 1, row 2 of the domain of size 8: "row" holds the COLUMN's element (the matrix is arithmetized transposed) and u_H belongs to it"""
    r, g = km.FR[377], km.r1cs_model.domain_gen(3)
    got = api.index_evals([1], [2], [3], [0], [-3], 4, 3)
    u_inv = pow(8 * pow(g, 7, r), -1, r)
    assert got["row"][:32] == zko.fr_pack([g]) and got["col"][:32] == zko.fr_pack([g * g % r]) and got["row_col"][:32] == zko.fr_pack([pow(g, 3, r)])
    assert got["val_a"][:32] == zko.fr_pack([3 * u_inv]) and got["val_b"][:32] == bytes(32) and got["val_c"][:32] == zko.fr_pack([-3 * u_inv])


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_anything_runs(ref, zko, api):
    g, one = ref.base(377, "generator"), zko.fr_pack([1])
    free0, _ = api.mem_info()
    for call, text in ((lambda: api.fixed_base_powers(375, g, one, 0, 4), "curve_id"), (lambda: api.fixed_base_powers(377, g, one, 0, (1 << 20) + 1), "out of range"),
                       (lambda: api.fixed_base_powers(377, g, one, 0, 4, chunk=(1 << 20) + 1), "out of range"), (lambda: api.fixed_base_powers(377, g, one, (1 << 64) - 5, 4), "2\\^64"),
                       (lambda: api.fixed_base_scalars(g, one * 4, chunk=(1 << 20) + 1), "out of range"),
                       (lambda: api.table_next(377, g * 3, 13, 0), "table copies"), (lambda: api.table_next(381, g * 3, 13, 20), "table copies"),
                       (lambda: api.table_next(377, g * 3, 1, 1), "window bits"), (lambda: api.table_next(377, b"", 13, 1), "count out of range"),
                       (lambda: api.build_window_tables(377, g * 3, 23), "window bits"), (lambda: api.build_window_tables(300, g * 3, 13), "curve_id"),
                       (lambda: api.convert_bases_te(b""), "n out of range"),
                       (lambda: api.index_evals([8], [0], [1], [0], [0], 4, 3), "index out of range"), (lambda: api.index_evals([0], [8], [1], [0], [0], 4, 3), "index out of range"),
                       (lambda: api.index_evals([0] * 17, [0] * 17, [1] * 17, [0] * 17, [0] * 17, 4, 3), "cnt must not exceed k"),
                       (lambda: api.index_evals([0], [0], [1], [0], [0], 21, 3), "lg_n and lg_k")):
        with pytest.raises(api.ZkAesError, match=text):
            call()
    out = C.create_string_buffer(96 * 4)
    assert api.lib().zkaes_fixed_base_powers(377, None, one, C.c_uint64(0), C.c_size_t(4), C.c_size_t(0), out) != 0 and b"null" in api.lib().zkaes_last_error()
    assert api.lib().zkaes_table_next(377, g, C.c_size_t(1), 13, 1, None) != 0 and b"null" in api.lib().zkaes_last_error()
    assert api.lib().zkaes_convert_bases_te(None, C.c_size_t(1), out) != 0 and b"null" in api.lib().zkaes_last_error()
    free1, _ = api.mem_info()
    assert free0 - free1 < 16 << 20, "device memory leaked on the refusal path: %d bytes" % (free0 - free1)
    assert api.fixed_base_powers(377, g, one, 0, 2) == g * 2                      # the good path afterwards: 1^i * G
