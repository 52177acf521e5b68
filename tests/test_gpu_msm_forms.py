"""GPU parity tests of the MSM in the FORMS THE PROVER CALLS IT (csrc/marlin.cpp), each through a kernel-level C entry point against the CPU oracle.  zkaes_msm,
zkaes_msm_table and zkaes_msm_table_srs (tests/test_gpu_kernels.py) take one scalar vector over one base range with table stride = n and offset 0; the prover never calls
the MSM like that.  Which entry point stands in for which call site:

  zkaes_class_sum         lagrange_commit   class_sum over int8 classes: the Lagrange-basis commitments of w, z_A, z_B (k_class_partials, k_quad_sum / k_sum_tree,
                                            k_class_result; the decline path and the re-arming of the flag word)
  zkaes_msm_second_bases  mpc_commit        a degree-bounded polynomial: one digit pass, msm_finish2 over the plain and the shifted powers, per-window and table mode
  zkaes_msm_pair          msm_opening_prepare (no tables)   two scalar vectors in ONE per-window Pippenger instance: the second k_digits launch with i_off = n1 and val_off
  zkaes_msm_table_pair    msm_opening_prepare (tables)      the same over window tables LONGER than the vectors: off1, off2 and n1 in k_digits_table / k_part_scatter;
                          msm_powers        with n2 = 0 and off1 > 0: one vector over a sub-range of the SRS (stride > n, offset != 0)

The reference is the oracle's MSM (zko_api_msm) over the points a case touches; bases are multiples of the generator (oracle_points), so they lie in the prime-order
subgroup the Edwards law needs.  Every comparison is BYTE EQUALITY of the affine result plus the infinity flag: no tolerance.  Shapes come from the constants of
kernels_msm.hip as READ from the source (tests/msm_model.py), and one vector of every multi-scalar case carries the edge scalars of the recoding that
tests/test_msm_model.py certifies for the window plan in force.  Large base arrays are tiled from 4,096 distinct points; the expected sum then adds up the scalars that
meet on one point before it asks the oracle."""
import ctypes as C
import random

import numpy as np
import pytest

import msm_model as M
from test_gpu_kernels import oracle_points

pytestmark = pytest.mark.gpu

K = M.constants()
R = M.R
CHUNK = K["CLS_CHUNK"]
DISTINCT = 4096
LAWS = [pytest.param(True, id="edwards"), pytest.param(False, id="weierstrass")]


class World:
    """4,096 distinct points of the prime-order subgroup, base arrays drawn from them by an index map, and the oracle's sum of what a case puts on them"""

    def __init__(self, zko):
        self.zko = zko
        self.points = np.frombuffer(oracle_points(zko, 377, DISTINCT, 0x4D534D), dtype=np.uint8).reshape(DISTINCT, 96)
        self.points.setflags(write=False)
        self.cache = {}

    def bases(self, ids):
        """the base array whose entry i is point ids[i]"""
        return np.ascontiguousarray(self.points[np.asarray(ids)])

    def tiled(self, n):
        return np.arange(n) % DISTINCT

    def msm(self, coeff):
        """oracle sum of coeff[p] * point p over the points with a non-zero coefficient mod r -> (xy, is_inf)"""
        items = sorted((int(p), int(c) % R) for p, c in coeff.items() if int(c) % R)
        out = C.create_string_buffer(96)
        if not items:
            return out.raw, True
        pts = np.ascontiguousarray(self.points[[p for p, _ in items]]).tobytes()
        inf = self.zko.lib().zko_api_msm(377, pts, self.zko.fr_pack([c for _, c in items]), C.c_size_t(len(items)), out)
        return out.raw, bool(inf)

    def expect_vals(self, vals, ids):
        """sum_i vals[i] * point ids[i] for small integers: the scalars are v mod r, only the non-zero positions go to the oracle"""
        acc = np.zeros(DISTINCT, dtype=np.int64)
        nz = np.nonzero(vals)[0]
        np.add.at(acc, np.asarray(ids)[nz], vals[nz].astype(np.int64))
        return self.msm({p: acc[p] for p in np.nonzero(acc)[0]})

    def expect_terms(self, terms, ids):
        """terms: (base index, canonical scalar) pairs"""
        coeff = {}
        for i, s in terms:
            p = int(ids[i])
            coeff[p] = (coeff.get(p, 0) + s) % R
        return self.msm(coeff)


@pytest.fixture(scope="module")
def world(zko):
    return World(zko)


def same(got_xy, got_inf, want, what):
    assert got_inf == want[1], "%s: infinity flag %s, the oracle says %s" % (what, got_inf, want[1])
    assert want[1] or got_xy == want[0], "%s: the sum differs from the oracle's" % what


# ---- class sums ------------------------------------------------------------------------------------------------------------------------------------------------------
WG = 64 * CHUNK                    # one workgroup of k_class_partials
MID = 256 * CHUNK                  # one mid-level block of the first sum
CLASS_SIZES = sorted({1, CHUNK - 1, CHUNK, CHUNK + 1, WG - 1, WG, WG + 1, MID - 1, MID, MID + 1})
BIG = 256 * 256 * CHUNK + 1        # the first size with more than 256 mid-level partials: the second-level sum loops (k_sum_tree; k_quad_sum already loops past RQ_QUADS)


def class_patterns(n, seed):
    """name -> int8 vector.  Dense patterns for n up to a few thousand (the oracle sums every non-zero position)"""
    rs = np.random.RandomState(seed)
    z = np.zeros(n, dtype=np.int8)
    pats = {"all zero": z.copy()}
    for v in (1, -1, 2, -2):
        pats["all %+d" % v] = np.full(n, v, dtype=np.int8)
    pats["mix of 0, +-1, +-2"] = rs.choice(np.array([0, 0, 1, -1, 1, 2, -2], dtype=np.int8), size=n)
    first, last = z.copy(), z.copy()
    first[0], last[n - 1] = -1, 2
    pats["one value at index 0"], pats["one value at index n - 1"] = first, last
    if n > CHUNK:
        one = z.copy()
        one[((n // CHUNK) // 2 + 1) * CHUNK - 1] = -2
        pats["one value at the last index of a chunk"] = one
    # one chunk whose only non-zero values are +-2 (its class-1 accumulator stays at the identity) among chunks of +-1
    only2 = rs.choice(np.array([0, 1, -1], dtype=np.int8), size=n)
    c0 = ((n - 1) // CHUNK // 2) * CHUNK
    only2[c0:c0 + CHUNK] = rs.choice(np.array([0, 2, -2, 2], dtype=np.int8), size=len(only2[c0:c0 + CHUNK]))
    only2[c0] = 2
    pats["a chunk with only +-2"] = only2
    return pats


def run_class_sums(api, world, ids, pats, edwards, prior=0):
    """every pattern through zkaes_class_sum, eight vectors per call on one workspace; every one must be ACCEPTED and equal the oracle's sum"""
    bases = world.bases(ids)
    names = list(pats)
    for b in range(0, len(names), 8):
        got = api.class_sum(bases, [pats[k] for k in names[b:b + 8]], edwards=edwards, prior_msm_points=prior)
        for k, (ok, xy, inf) in zip(names[b:b + 8], got):
            assert ok, "class_sum declined '%s' (n = %d): nothing in it is out of range or degenerate" % (k, len(ids))
            same(xy, inf, world.expect_vals(pats[k], ids), "class sum '%s', n = %d" % (k, len(ids)))


@pytest.mark.parametrize("edwards", LAWS)
@pytest.mark.parametrize("n", CLASS_SIZES)
def test_class_sums_at_the_chunk_workgroup_and_block_boundaries(world, api, edwards, n):
    run_class_sums(api, world, world.tiled(n), class_patterns(n, 100 + n), edwards)


@pytest.mark.parametrize("edwards", LAWS)
def test_class_sums_with_more_than_256_mid_level_partials(world, api, edwards):
    """n = 256 x 256 x CLS_CHUNK + 1: 257 mid-level partials, so the second-level sum walks more inputs than it has lanes.  Tiled bases, a few hundred non-zero values."""
    n, ids = BIG, world.tiled(BIG)
    rs = np.random.RandomState(7)
    z = np.zeros(n, dtype=np.int8)
    pos = np.unique(np.concatenate([rs.randint(0, n, size=300), [0, n - 1, n - 2, CHUNK - 1, CHUNK, MID - 1, MID, 256 * MID - 1, 256 * MID - CHUNK]]))
    mix, twos = z.copy(), z.copy()
    mix[pos] = rs.choice(np.array([1, -1, 2, -2], dtype=np.int8), size=len(pos))
    twos[pos[::3]] = rs.choice(np.array([2, -2], dtype=np.int8), size=len(pos[::3]))
    first, last, chunk_last, cancel = z.copy(), z.copy(), z.copy(), z.copy()
    first[0], last[n - 1], chunk_last[200 * MID + 5 * CHUNK - 1] = 1, -1, 2
    cancel[12345], cancel[12345 + 77 * DISTINCT] = 1, -1                    # the same point in two far-apart chunks
    pats = {"all zero": z, "sparse mix": mix, "sparse +-2 only": twos, "one value at index 0": first, "one value at index n - 1": last,
            "one value at the last index of a chunk": chunk_last, "P and -P far apart": cancel}
    run_class_sums(api, world, ids, pats, edwards)
    assert world.expect_vals(cancel, ids)[1]


@pytest.mark.parametrize("edwards", LAWS)
def test_class_sums_of_a_point_that_meets_itself(world, api, edwards):
    """The same point at two indices.  In DIFFERENT chunks the partial sums meet in the tree, whose addition is complete on both laws: P - P is infinity, P + P is 2 P.
    In ONE chunk the Edwards law's unified addition takes P + P and P - P in its stride; the Weierstrass law's mixed addition cannot (madd28 returns false for P = +-Q),
    raises the flag and class_sum DECLINES -- pinned here: a decline or the right sum is the contract, a wrong point is the failure."""
    n = 3 * CHUNK + 5
    ids = np.arange(n)
    ids[5] = ids[2]                                  # chunk 0 holds point 2 twice
    ids[2 * CHUNK + 1] = ids[CHUNK + 4]              # chunks 1 and 2 share a point
    a, b = CHUNK + 4, 2 * CHUNK + 1

    def vec(**at):
        v = np.zeros(n, dtype=np.int8)
        for k, val in at.items():
            v[int(k[1:])] = val
        return v

    far = {"P - P across chunks": vec(**{"i%d" % a: 1, "i%d" % b: -1}), "P + P across chunks": vec(**{"i%d" % a: 1, "i%d" % b: 1}),
           "2 P - 2 P across chunks, among others": vec(i0=1, i7=-2, **{"i%d" % a: 2, "i%d" % b: -2})}
    run_class_sums(api, world, ids, far, edwards)
    assert world.expect_vals(far["P - P across chunks"], ids)[1]
    near = {"P + P in one chunk": vec(i2=1, i5=1), "P - P in one chunk, among others": vec(i2=1, i5=-1, i7=1, i9=-2), "2 P + 2 P in one chunk": vec(i2=2, i5=2),
            "P - P alone in one chunk": vec(i2=-1, i5=1)}
    if edwards:
        run_class_sums(api, world, ids, near, edwards)
        assert world.expect_vals(near["P - P alone in one chunk"], ids)[1]
    else:
        got = api.class_sum(world.bases(ids), list(near.values()), edwards=False)
        assert [ok for ok, _, _ in got] == [False] * len(near), "the Weierstrass class sum is pinned to DECLINE a point that meets itself or its negative inside a chunk"


@pytest.mark.parametrize("edwards", LAWS)
@pytest.mark.parametrize("where", ["first index", "last index", "inside the tail chunk"])
def test_class_sum_declines_out_of_range_values_and_the_flag_word_rearms(world, api, edwards, where):
    """3, -3, 127 and -128 are refused wherever they sit, and the NEXT vector on the same workspace is accepted with the right sum: k_class_result re-armed the flag word.
    Clean vectors before, between and after two declining ones."""
    n = WG + CHUNK + 6                                                     # two workgroups; the tail chunk holds 6 values
    at = {"first index": 0, "last index": n - 1, "inside the tail chunk": n - 4}[where]
    ids = world.tiled(n)
    bases = world.bases(ids)
    rs = np.random.RandomState(n + at)
    clean = [rs.choice(np.array([0, 1, -1, 2, -2], dtype=np.int8), size=n) for _ in range(3)]
    want = [world.expect_vals(v, ids) for v in clean]
    for bad_a, bad_b in ((3, -3), (127, -128)):
        bad = []
        for x in (bad_a, bad_b):
            v = clean[1].copy()
            v[at] = x
            bad.append(v)
        got = api.class_sum(bases, [clean[0], bad[0], clean[1], bad[1], clean[2]], edwards=edwards)
        assert [ok for ok, _, _ in got] == [True, False, True, False, True], "values %d and %d at the %s" % (bad_a, bad_b, where)
        for i, j in ((0, 0), (2, 1), (4, 2)):
            same(got[i][1], got[i][2], want[j], "the clean vector after a declined one (%d, %d at the %s)" % (bad_a, bad_b, where))


@pytest.mark.parametrize("edwards", LAWS)
@pytest.mark.parametrize("prior", [0, DISTINCT])
def test_class_sums_on_a_workspace_another_msm_sized(world, api, edwards, prior):
    """a lone first call grows the scratch itself; behind a generic MSM of 4,096 points (26 windows x 512 buckets) the class sums carve theirs from that bucket array"""
    n = MID + 1
    pats = class_patterns(n, 5)
    run_class_sums(api, world, world.tiled(n), {k: pats[k] for k in ("mix of 0, +-1, +-2", "all -2", "a chunk with only +-2")}, edwards, prior=prior)


# ---- two scalar vectors in one Pippenger instance ------------------------------------------------------------------------------------------------------------------------
def scalar_vectors(plan, n1, n2, relation, shared_from, edge_in, seed):
    """(canonical scalars of vector 1, of vector 2): one carries the plan's certified edge scalars (all of them, twice over, where it is long enough), the other is random
    with 0, 1 and r - 1 in front.  relation "equal" / "negated": where the ranges overlap (vector 1 from `shared_from` on), vector 2 repeats / negates vector 1's scalars."""
    rng = random.Random(seed)
    edges = list(M.edge_scalars(plan).values())

    def rand_vec(n):
        return ([0, 1, R - 1] + [rng.randrange(R) for _ in range(n)])[:n]

    def edge_vec(n):
        lead = [edges[i % len(edges)] for i in range(min(n, 2 * len(edges)))]
        return lead + [rng.randrange(R) for _ in range(n - len(lead))]

    s1 = edge_vec(n1) if (edge_in == 1 or n2 == 0) and n1 else rand_vec(n1)
    s2 = edge_vec(n2) if (edge_in == 2 or n1 == 0) and n2 else rand_vec(n2)
    if relation:
        assert shared_from + len(edges) <= n1, "the shared stretch must hold edge scalars too"
        rot = edge_vec(n1)
        s1 = rot[-shared_from:] + rot[:-shared_from] if shared_from else rot           # the edge scalars start where the overlap starts
        for j in range(min(n2, n1 - shared_from)):
            s2[j] = s1[shared_from + j] if relation == "equal" else (R - s1[shared_from + j]) % R
    return s1, s2


#             name                      n1    n2  val_off2  relation  edge scalars in
PAIR_CASES = [("one vector",            512,    0,     0,  None,      1),
              ("second vector only",      0,  513,    37,  None,      2),
              ("one and one",             1,    1,     1,  None,      1),
              ("ranges with a gap",     500,  524,   700,  None,      2),
              ("adjacent ranges",       512,  513,   512,  None,      1),
              ("overlap, random",       300,  212,   200,  None,      2),
              ("overlap, equal",        300,  213,   100,  "equal",   1),
              ("overlap, negated",      600,  424,   400,  "negated", 1),
              ("past 2^14",            8192, 8193,  8000,  None,      2)]


def test_the_pair_cases_cover_the_window_steps():
    assert sorted(set(n1 + n2 for _, n1, n2, _, _, _ in PAIR_CASES)) == sorted(M.PAIR_TOTALS)
    assert sorted(set(M.window_bits_for(n1 + n2) for _, n1, n2, _, _, _ in PAIR_CASES)) == [7, 8, 9, 13]


@pytest.mark.parametrize("edwards", LAWS)
@pytest.mark.parametrize("case", PAIR_CASES, ids=[c[0] for c in PAIR_CASES])
def test_two_scalar_vectors_share_one_per_window_instance(world, zko, api, edwards, case):
    name, n1, n2, off2, relation, edge_in = case
    plan = M.per_window_plan(n1 + n2)
    s1, s2 = scalar_vectors(plan, n1, n2, relation, off2, edge_in, 1000 + n1 + n2)
    ids = world.tiled(max(n1, off2 + n2) + 5)
    want = world.expect_terms([(i, s) for i, s in enumerate(s1)] + [(off2 + j, s) for j, s in enumerate(s2)], ids)
    xy, inf = api.msm_pair(world.bases(ids), zko.fr_pack(s1), zko.fr_pack(s2), off2, edwards=edwards)
    same(xy, inf, want, "%s (n1 = %d, n2 = %d, val_off2 = %d, %s)" % (name, n1, n2, off2, plan))


# ---- two vectors and offsets in table mode -------------------------------------------------------------------------------------------------------------------------------
def at_threshold(c):
    """the fewest scalars whose (point, window) pairs reach the partition's threshold under c window bits"""
    return -(-K["PART_MIN_PAIRS"] // M.table_layout(c)[0])


N20, N17 = at_threshold(20), at_threshold(17)
#              name                                          stride        n1   off1            n2          off2   c  partition
TABLE_CASES = [("radix sort, second range ends the table",     1200,      400,  100,           500,          700, 20, False),
               ("one vector at an offset, ends the table",     1200,      600,  600,             0,            0, 17, False),
               ("second vector only",                          1200,        0,    0,           700,          333, 12, False),
               ("one pair below the threshold",          N20 + 1000,     3000,   17,  N20 - 1 - 3000,       4000, 20, False),
               ("partition at its threshold, 20 bits",   N20 + 1001,     3000,   17,      N20 - 3000,       4001, 20, True),
               ("partition, 17 bits, overlapping ranges",      6100,     3000,   17,  N17 + 30 - 3000,      2500, 17, True),
               ("17 windows stay on the radix sort",     N20 + 1001,     3000,   17,      N20 - 3000,       4001, 15, False)]


@pytest.mark.parametrize("edwards", LAWS)
@pytest.mark.parametrize("case", TABLE_CASES, ids=[c[0] for c in TABLE_CASES])
def test_two_scalar_vectors_at_offsets_into_longer_window_tables(world, zko, api, edwards, case):
    name, stride, n1, off1, n2, off2, c, partition = case
    assert off1 + n1 <= stride and off2 + n2 <= stride and stride > n1 + n2
    assert M.partition_accepts(c, (n1 + n2) * M.table_layout(c)[0], K) == partition, "the case no longer takes the grouping path it is named for"
    s1, s2 = scalar_vectors(M.table_plan(c), n1, n2, None, 0, 1 if c != 20 else 2, 2000 + stride + c)
    ids = world.tiled(stride)
    want = world.expect_terms([(off1 + i, s) for i, s in enumerate(s1)] + [(off2 + j, s) for j, s in enumerate(s2)], ids)
    xy, inf = api.msm_table_pair(world.bases(ids), zko.fr_pack(s1), off1, zko.fr_pack(s2), off2, c, edwards=edwards)
    same(xy, inf, want, "%s (stride %d, n1 = %d at %d, n2 = %d at %d, %d bits)" % (name, stride, n1, off1, n2, off2, c))


def test_ranges_outside_the_bases_are_refused_and_nothing_leaks(world, zko, api):
    """off + n > stride is refused with the library's own message before anything is allocated; an error in the MIDDLE of a call (a base of order 2 that the Edwards
    conversion refuses once the bases, the values and the stream exist) gives everything back; the good path works afterwards"""
    n = 1200
    ids = world.tiled(n)
    bases = world.bases(ids)
    s = zko.fr_pack([random.Random(1).randrange(R) for _ in range(300)])
    q = zko.FQ[377]
    order2 = bases.copy()
    order2[7, :48] = np.frombuffer(((q - 1) * pow(2, 384, q) % q).to_bytes(48, "little"), dtype=np.uint8)       # (-1, 0) on y^2 = x^3 + 1
    order2[7, 48:] = 0
    ones = np.ones(n, dtype=np.int8)
    api.msm_table_pair(bases, s, 10, s, 700, 12, edwards=True)                # warm the runtime's own pools before the first reading
    free0, _ = api.mem_info()
    for _ in range(3):
        for call in (lambda: api.msm_table_pair(bases, s, n - 299, b"", 0, 20), lambda: api.msm_table_pair(bases, s, 0, s, n - 299, 20, edwards=False),
                     lambda: api.msm_table_pair(bases, b"", n + 1, b"", 0, 20), lambda: api.msm_second_bases(bases, s, 500, 401, 20)):
            with pytest.raises(api.ZkAesError, match="msm_table: range exceeds the table"):
                call()
        for call in (lambda: api.msm_pair(bases, s, s, n - 299), lambda: api.msm_pair(bases[:299], s, b"", 0), lambda: api.msm_second_bases(bases, s, 500, 401, 0)):
            with pytest.raises(api.ZkAesError, match="range exceeds the bases"):
                call()
        for bits in (1, 23, -3):
            with pytest.raises(api.ZkAesError, match="window bits"):
                api.msm_table_pair(bases, s, 0, b"", 0, bits)
        with pytest.raises(api.ZkAesError, match="1..8 value vectors"):
            api.class_sum(bases, [ones] * 9)
        with pytest.raises(api.ZkAesError, match="1..8 value vectors"):
            api.class_sum(bases, [])
        with pytest.raises(api.ZkAesError, match="at most n points"):
            api.class_sum(bases, [ones], prior_msm_points=n + 1)
        out, inf = C.create_string_buffer(192), (C.c_int * 2)()
        assert api.lib().zkaes_msm_pair(None, C.c_size_t(4), s, C.c_size_t(4), None, C.c_size_t(0), C.c_size_t(0), 1, out, inf) != 0 and b"null" in api.lib().zkaes_last_error()
        assert api.lib().zkaes_class_sum(bases.ctypes.data_as(C.c_void_p), C.c_size_t(n), None, 1, 1, C.c_size_t(0), inf, out, inf) != 0 and b"null" in api.lib().zkaes_last_error()
        with pytest.raises(api.ZkAesError, match="order 2 or 4"):
            api.class_sum(order2, [ones] * 8, edwards=True)
        with pytest.raises(api.ZkAesError, match="order 2 or 4"):
            api.msm_second_bases(order2, s, 100, 50, 20)
    free1, _ = api.mem_info()
    assert free0 - free1 < 16 << 20, "device memory leaked on the error path: %d bytes" % (free0 - free1)
    xy, inf = api.msm_table_pair(bases, s, 10, s, 700, 12, edwards=True)
    same(xy, inf, world.expect_terms([(10 + i, v) for i, v in enumerate(zko.fr_unpack(s))] + [(700 + i, v) for i, v in enumerate(zko.fr_unpack(s))], ids), "the good path after the refusals")


# ---- one digit pass, two base ranges -------------------------------------------------------------------------------------------------------------------------------------
#                 n                       window bits
SECOND_CASES = [(n, 0) for n in M.SECOND_BASES_SIZES] + [(700, 20), (N20 + 9, 20)]


@pytest.mark.parametrize("shift", ["1", "end"])
@pytest.mark.parametrize("n,c", SECOND_CASES)
def test_one_digit_pass_over_the_plain_and_the_shifted_bases(world, zko, api, n, c, shift):
    """msm_finish2: per-window mode at 512 points (2 x 37 window sums: more than one reduction returns, so one base array after the other), 513 (2 x 32: exactly the limit)
    and 1,025 (2 x 29); table mode below and above the partition's threshold.  Both sums against two independent oracle MSMs."""
    if c == 0:
        nwin = M.per_window_plan(n).nwin
        assert (2 * nwin > K["MAX_WSUMS"]) == (n == 512) and (2 * nwin == K["MAX_WSUMS"]) == (n == 513)
    else:
        assert M.partition_accepts(c, n * M.table_layout(c)[0], K) == (n != 700)
    nbases, off = n + 300, 100
    sh = 1 if shift == "1" else nbases - off - n
    s, _ = scalar_vectors(M.table_plan(c) if c else M.per_window_plan(n), n, 0, None, 0, 1, 3000 + n + c)
    ids = world.tiled(nbases)
    got = api.msm_second_bases(world.bases(ids), zko.fr_pack(s), off, sh, c)
    for which, base0 in enumerate((off, off + sh)):
        same(got[which][0], got[which][1], world.expect_terms([(base0 + i, v) for i, v in enumerate(s)], ids), "%s sum (n = %d, %d bits, shift %d)" % (("plain", "shifted")[which], n, c, sh))


@pytest.mark.parametrize("n,c", [(513, 0), (700, 20)])
def test_all_zero_scalars_give_infinity_over_both_base_ranges(world, api, n, c):
    got = api.msm_second_bases(world.bases(world.tiled(n + 50)), bytes(32 * n), 3, 40, c)
    assert [inf for _, inf in got] == [True, True]
