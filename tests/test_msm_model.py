"""CPU checks of tests/msm_model.py: the window plans against the numbers the source states, the recoding against the integers it must represent, and a certificate, for
every plan the GPU tests run, that each constructed edge scalar really reaches the edge it is named for (tests/test_gpu_msm_forms.py)."""
import random

import pytest

import msm_model as M

K = M.constants()
PLANS = M.gpu_test_plans()


def test_the_constants_the_case_lists_are_derived_from(zko):
    """what the shapes of tests/test_gpu_msm_forms.py assume about kernels_msm.hip as it stands"""
    assert M.R == zko.R377 and (1 << 252) < M.R < (1 << 253)
    assert K["CLS_CHUNK"] >= 2 and K["RQ_QUADS"] == 64 and K["RQ_QUADS"] < 256          # the Edwards second-level sum loops past 64 partials, the Weierstrass one past 256
    assert 256 * 256 * K["CLS_CHUNK"] + 1 < 1 << 26                                     # the size with 257 mid-level partials stays a sparse, tiled case of ~10^6 points
    assert K["BUCKET_CAP_TABLE"] >= 64 and K["PART_FINE_BITS"] == 9 and K["PART_WBITS"] == 4 and K["PART_NBIN_MAX"] == 1024
    # msm_finish2's threshold sits between n = 512 and n = 513, and 1,025 points are comfortably below it
    nwin = [M.per_window_plan(n).nwin for n in M.SECOND_BASES_SIZES]
    assert 2 * nwin[0] > K["MAX_WSUMS"] and 2 * nwin[1] == K["MAX_WSUMS"] and 2 * nwin[2] < K["MAX_WSUMS"] - 4, (nwin, K["MAX_WSUMS"])
    # table mode: 20 and 17 bits go through the partition from PART_MIN_PAIRS pairs on, 15 bits (17 windows) never do
    big = K["PART_MIN_PAIRS"]
    assert M.partition_accepts(20, big, K) and M.partition_accepts(17, big, K) and not M.partition_accepts(15, 1 << 30, K)
    assert not M.partition_accepts(20, big - 1, K) and not M.partition_accepts(17, big - 1, K)


def test_window_plans_match_the_numbers_the_source_states():
    assert M.table_layout(20) == (13, 20, 7)                                             # "254 = 7 x 20 + 6 x 19 for c = 20"
    p = M.table_plan(20)
    assert [w for _, w in p.windows] == [20] * 7 + [19] * 6 and p.offset(7) == 140 and p.offset(12) == 235
    assert M.table_layout(17) == (15, 17, 14) and M.table_layout(15) == (17, 15, 16) and M.table_layout(16) == (16, 16, 14)
    assert M.table_layout(2) == (127, 2, 127)                                            # no remainder: every window c_hi wide
    for c in range(2, 23):
        assert sum(w for _, w in M.table_plan(c).windows) == 254
    # per-window mode: c = clamp(lg - 2, 7, 17), nwin = ceil(254 / c): "<= 37 windows"
    assert [(M.window_bits_for(n), M.per_window_plan(n).nwin) for n in (1, 512, 513, 1024, 1025, 1 << 14, (1 << 14) + 1, 1 << 19, 1 << 25)] == \
        [(7, 37), (7, 37), (8, 32), (8, 32), (9, 29), (12, 22), (13, 20), (17, 15), (17, 15)]


@pytest.mark.parametrize("plan", PLANS, ids=repr)
def test_recoding_represents_the_scalar(plan):
    rng = random.Random(len(plan.windows))
    scalars = [0, 1, 2, M.R - 1, M.R - 2, (1 << 252) - 1, 1 << 252] + [rng.randrange(M.R) for _ in range(300)] + list(M.edge_scalars(plan).values())
    for s in scalars:
        d = M.recode(s, plan)
        assert M.digits_value(d, plan) == s, hex(s)
        assert d[-1][2] == 0, "a carry leaves the top window: %x" % s
        for j, (v, skip, carry) in enumerate(d):
            assert -plan.half(j) < v <= plan.half(j) and skip == (v == 0) and carry in (0, 1)
            field, carry_in = (s >> plan.offset(j)) & ((1 << plan.width(j)) - 1), d[j - 1][2] if j else 0
            assert field + carry_in == v + (carry << plan.width(j))                     # the window's own identity: what comes in is what goes out


@pytest.mark.parametrize("plan", PLANS, ids=repr)
def test_the_top_window_never_reaches_half(plan):
    """a scalar below r leaves the top window at most (r - 1) >> offset, + 1 with a carry: below `half`, so the top digit never recodes, no carry is lost, and "v > half"
    and "v >= half" could only differ in the SUM there: below the top, -half with a carry into the next window and +half are the same integer, so both digit strings
    represent the scalar and sum_w digit_w 2^offset(w) P is the same point.  (A test that compares sums cannot tell the two comparisons apart, and need not.)"""
    top = plan.nwin - 1
    assert ((M.R - 1) >> plan.offset(top)) + 1 < plan.half(top)
    rng = random.Random(plan.nwin)
    for s in list(M.edge_scalars(plan).values()) + [M.R - 1, 0] + [rng.randrange(M.R) for _ in range(100)]:
        a, b = M.recode(s, plan), M.recode(s, plan, recode_at_half=True)
        assert M.digits_value(b, plan) == s and b[-1][2] == 0
        assert M.digits_value(a, plan) == s and all(1 <= abs(v) <= plan.half(j) for j, (v, skip, _) in enumerate(b) if not skip)      # every digit still names a bucket of its window


@pytest.mark.parametrize("plan", PLANS, ids=repr)
def test_every_edge_scalar_reaches_the_edge_it_is_named_for(plan):
    e = M.edge_scalars(plan)
    top = plan.nwin - 1
    d = {name: M.recode(s, plan) for name, s in e.items()}
    for name, s in e.items():
        assert 0 <= s < M.R and M.digits_value(d[name], plan) == s, name
    # a digit of exactly half, kept positive, and no carry anywhere
    assert sum(1 for j, (v, _, _) in enumerate(d["half"]) if v == plan.half(j)) >= plan.nwin - 2
    assert all(c == 0 for _, _, c in d["half"])
    # half + 1 recodes with a carry: window 0 gives -(half - 1); in half_then_carry every further non-empty window reaches half + 1 only through the carry
    for name in ("half_plus_one", "half_then_carry"):
        assert d[name][0] == (-(plan.half(0) - 1), False, 1), name
    hc = d["half_then_carry"]
    chained = [j for j in range(1, plan.nwin) if hc[j][0] == -(plan.half(j) - 1) and hc[j - 1][2] == 1 and ((e["half_then_carry"] >> plan.offset(j)) & ((1 << plan.width(j)) - 1)) == plan.half(j)]
    assert len(chained) >= plan.nwin - 3
    # the all-ones scalar: a zero digit with SKIP and an outgoing carry in every full window but the first
    ao = d["all_ones"]
    assert ao[0] == (-1, False, 1)
    zero_with_carry = [j for j in range(1, plan.nwin) if ao[j] == (0, True, 1)]
    assert len(zero_with_carry) >= plan.nwin - 3 and all(plan.offset(j) + plan.width(j) <= 252 for j in zero_with_carry)
    # a carry that reaches the top window: the top field is zero, the top digit is 1
    ct = d["carry_to_top"]
    assert (e["carry_to_top"] >> plan.offset(top)) == 0 and ct[top] == (1, False, 0) and ct[top - 1][2] == 1
    assert all(ct[j] == (0, True, 1) for j in range(1, top))
    # powers of two at the window and limb boundaries: one digit 1 (or a high bit of a straddling window); 2^k - 1 is -1 and a carry chain that ends in +1 at k's window
    ks = sorted(int(name.split("_")[1]) for name in e if name.startswith("pow2_"))
    assert set(plan.offset(j) for j in range(1, plan.nwin) if plan.offset(j) <= 252) <= set(ks)
    for limb in range(1, 8):
        straddled = any(off < 32 * limb < off + w for off, w in plan.windows)
        assert (32 * limb in ks) == (straddled or 32 * limb in [plan.offset(j) for j in range(plan.nwin)])
    for k in ks:
        nz = [(j, v) for j, (v, _, _) in enumerate(d["pow2_%d" % k]) if v]
        assert len(nz) == 1 and nz[0][1] == 1 << (k - plan.offset(nz[0][0])), k          # (the top bit of a straddling window is the digit `half`: it stays positive)
        m1 = d["pow2m1_%d" % k]
        assert m1[0] == (-1, False, 1) and sum(1 for v, skip, c in m1 if skip and c) == sum(1 for j in range(1, plan.nwin) if plan.offset(j) + plan.width(j) <= k), k
        assert sum(1 for v, _, _ in m1 if v > 0) == 1
