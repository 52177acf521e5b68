"""GPU tests of MSM SEQUENCES ON ONE REUSED WORKSPACE, as the prover runs them.  Every other kernel-level MSM test makes a workspace, runs one MSM on it and drops it; a
prover context (csrc/marlin.cpp Lane::ws) and the batch verifier keep one MsmWorkspace alive and push class sums, per-window pairs, table pairs and msm_finish2 calls of
different sizes and window plans through it back to back.  The workspace is stateful by design (csrc/kernels_msm.hip):

  ctrl[0]              the overflow list's counter, armed at zero between MSMs (k_order_scan re-arms it); ctrl[1], ctrl[2] keep the last list's length and segment total
  ctrl[3]              the class-sum flag word, re-armed by k_class_result
  deferred_count[1]    the tail kernel's workgroup ticket, re-armed by its taker; the Weierstrass law memsets both words before an accumulation, the Edwards law never does
  start, end, ovf_slot written per bucket with nothing memset beforehand
  every buffer         only ever grows: a small MSM runs inside the keys, values, ranges, orders, overflow lists and accumulators of a larger one before it

All of that matters only when the overflow list, the deferred list or the class-sum flags are non-empty -- skewed scalars, repeated bases, declined class vectors -- and
whole proofs, the one place a workspace is reused otherwise, have uniform scalars.  zkaes_msm_sequence (include/zkaes.h) runs a list of steps on ONE workspace and ONE
stream and returns every step's result; with `poison` it fills the accumulator buffers (never the armed words or the index-bearing buffers, whose stale contents are the
state under test) with 0xAB bytes before every step but the first.

The reference is the oracle's MSM (zko_api_msm) over exactly the points and scalars a step touches (class sums: the values mod r over their non-zero positions).  EVERY
step of EVERY sequence is compared: byte equality of the affine point plus the infinity flag, no tolerance.  Every sequence runs with poison off and on, and in both laws
except the mixed-law one (msm_finish2 exists on the Edwards law only: its steps keep that law in the Weierstrass runs).  A reference is computed once and shared.

Bases: 40,000 distinct points of the prime-order subgroup, so that the deferred list stays empty except where a step asks for repeats -- the 64 copies of one further
point behind them, outside every range the other steps use.  Sizes come from the constants of kernels_msm.hip as READ from the source (tests/msm_model.py)."""
import ctypes as C
import re

import numpy as np
import pytest

import msm_model as M
from test_gpu_kernels import fast_fr_mont, oracle_points

pytestmark = pytest.mark.gpu

K = M.constants()
R = M.R
CAP = int(re.search(r"\bBUCKET_CAP = (\d+)\b", open(M.SOURCE).read()).group(1))      # the per-window cap, read from the source as msm_model.constants() reads the others
CHUNK = K["CLS_CHUNK"]
N = 40_000                                   # distinct points
RUN = 64                                     # copies of one more point behind them: the Weierstrass law defers every addition after the first
NBASES = N + RUN
N_UNI = (1 << 14) + 7                        # the sizing step: c = 13, 20 windows x 4,096 buckets
N_SKEW = max(10_000, 3 * CAP + 3 * 64 + 1)   # per-window: every digit of one or of three distinct scalars fills a bucket beyond BUCKET_CAP
N_CLS = 64 * CHUNK + CHUNK + 6               # two workgroups of k_class_partials, a tail chunk of 6 values
LAWS = [pytest.param(True, id="edwards"), pytest.param(False, id="weierstrass")]
POISON = [pytest.param(False, id="plain"), pytest.param(True, id="poisoned")]


def table_cap(n, c):
    """msm_prepare_table's per-lane cap for n scalars under c window bits"""
    nwin, c_hi, _ = M.table_layout(c)
    cap = K["BUCKET_CAP_TABLE"]
    while cap < 2 * (n * nwin // (1 << (c_hi - 1))) + 64:
        cap <<= 1
    return cap


def takes_partition(n, c):
    return M.partition_accepts(c, n * M.table_layout(c)[0], K)


def test_the_shapes_reach_the_paths_they_are_named_for():
    """(no GPU work: the constants of kernels_msm.hip against the sizes below)"""
    assert N_SKEW <= N and N_SKEW // 3 > CAP, "three distinct scalars no longer overflow a per-window bucket"
    assert M.window_bits_for(N_UNI) > M.window_bits_for(N_SKEW) > M.window_bits_for(1000) > M.window_bits_for(33), "the per-window steps no longer shrink c, nwin and the bucket count"
    assert 2 * M.per_window_plan(N_SKEW).nwin <= K["MAX_WSUMS"], "msm_finish2 over the skewed vector would run its base arrays one after the other: the ticket is no longer taken twice in one MSM"
    # (one scalar's 22 digits fill up to 22 buckets with all N points each: ~39 overflow segments per bucket, the list's segments in more than two workgroups of the tail kernel)
    assert 20_000 // 3 > table_cap(20_000, 16) and (N - 1) // table_cap(N, 12) * (M.table_layout(12)[0] // 2) > 2 * 64, "the skewed table steps no longer overflow (the second one across several 64-segment workgroups)"
    # (5,000 scalars under 16 bits are 80,000 pairs: above the partition's threshold, whatever the older tests' comments say; 3,000 stay on the radix sort)
    assert [takes_partition(n, c) for n, c in ((3_000, 16), (5_000, 16), (9_000, 18), (9_000, 15), (20_000, 16), (N, 12), (1_200, 18))] == [False, True, True, False, True, False, False]


# ---- the world: bases, scalars, class values, and the oracle's sums over ranges of them ---------------------------------------------------------------------------------
U0, S1, S3, T3 = 0, N, 2 * N, 2 * N + 20_000          # scalar blob: 40,000 uniform | 40,000 x one value | 20,000 cycling through three values | 64 x the scalar 3
V_A, V_BAD, V_B, V_C = 0, N_CLS, 2 * N_CLS, 3 * N_CLS  # class values: three clean vectors and one with a value out of range


class World:
    def __init__(self, zko):
        self.zko = zko
        pts = np.frombuffer(oracle_points(zko, 377, N + 1, 0x5EC0), dtype=np.uint8).reshape(N + 1, 96)
        assert len(np.unique(pts, axis=0)) == N + 1, "the oracle's points are not distinct"
        self.bases = np.ascontiguousarray(np.concatenate([pts[:N], np.repeat(pts[N:], RUN, axis=0)]))
        self.bases.setflags(write=False)
        uni = bytearray(fast_fr_mont(N, 0x5EC1))
        uni[0:32], uni[32:64], uni[64:96] = bytes(32), zko.fr_pack([1]), zko.fr_pack([R - 1])
        skew = [int.from_bytes(np.random.RandomState(0x5EC2 + i).bytes(31), "little") for i in range(4)]
        self.scalars = bytes(uni) + zko.fr_pack(skew[:1]) * N + (zko.fr_pack(skew[1:]) * (20_000 // 3 + 1))[:32 * 20_000] + zko.fr_pack([3]) * RUN
        assert len(self.scalars) == 32 * (T3 + RUN)
        rs = np.random.RandomState(0x5EC3)
        clean = [rs.choice(np.array([0, 0, 1, -1, 1, 2, -2], dtype=np.int8), size=N_CLS) for _ in range(3)]
        bad = clean[0].copy()
        bad[N_CLS - 4] = 3                                   # inside the tail chunk
        self.vals = np.concatenate([clean[0], bad, clean[1], clean[2]])
        self.cache = {}

    def msm(self, key):
        """key: ("s", (first base, first scalar, n), ...) -- sum of scalars[first scalar + i] * bases[first base + i] over the ranges; ("c", first base, first value, n) --
        the class sum of that value range -> (xy, is_inf), from the oracle, once per key"""
        if key not in self.cache:
            if key[0] == "s":
                pts = b"".join(self.bases[b:b + n].tobytes() for b, _, n in key[1:])
                sc = b"".join(self.scalars[32 * s:32 * (s + n)] for _, s, n in key[1:])
            else:
                _, b, v, n = key
                vals = self.vals[v:v + n]
                nz = np.nonzero(vals)[0]
                pts = np.ascontiguousarray(self.bases[b + nz]).tobytes()
                sc = self.zko.fr_pack([int(x) % R for x in vals[nz]])
            out = C.create_string_buffer(96)
            n = len(sc) // 32
            assert len(pts) == 96 * n
            inf = self.zko.lib().zko_api_msm(377, pts, sc, C.c_size_t(n), out) if n else 1
            self.cache[key] = (out.raw, bool(inf))
        return self.cache[key]


@pytest.fixture(scope="module")
def world(zko):
    return World(zko)


# ---- steps: what to run and what to expect of it -----------------------------------------------------------------------------------------------------------------------
class Step:
    def __init__(self, what, fields, outs, refused=None, declined=False):
        self.what, self.fields, self.outs, self.refused, self.declined = what, fields, outs, refused, declined


def ranges(*r):
    return ("s",) + tuple((b, s, n) for b, s, n in r if n)


def win(e, n1, s1, base=0, n2=0, off2=0, s2=0, what=None, refused=None):
    """per-window single or pair: msm_prepare(n1, n2, val_off2) + msm_finish on the bases from `base` on"""
    return Step(what or "per-window %d + %d at base %d" % (n1, n2, base), dict(kind=0, edwards=int(e), n1=n1, off1=base, scal1=s1, n2=n2, off2=off2, scal2=s2),
                [ranges((base, s1, n1), (base + off2, s2, n2))], refused)


def tab(e, c, n1, off1, s1, n2=0, off2=0, s2=0, what=None, refused=None):
    """table single or pair: msm_prepare_table(stride = all the bases) + msm_finish"""
    return Step(what or "table c=%d, %d at %d + %d at %d" % (c, n1, off1, n2, off2), dict(kind=1, edwards=int(e), window_bits=c, n1=n1, off1=off1, scal1=s1, n2=n2, off2=off2, scal2=s2),
                [ranges((off1, s1, n1), (off2, s2, n2))], refused)


def second(c, n, off, shift, s, what=None):
    """one prepared state, msm_finish2 over the plain and the shifted range (Edwards law)"""
    return Step(what or "second bases c=%d, %d at %d and %d further" % (c, n, off, shift), dict(kind=2, edwards=1, window_bits=c, n1=n, off1=off, scal1=s, shift=shift),
                [ranges((off, s, n)), ranges((off + shift, s, n))])


def cls(e, v, base=0, declined=False):
    return Step("class sum of the values at %d over the bases from %d on" % (v, base), dict(kind=3, edwards=int(e), n1=N_CLS, off1=base, scal1=v), [("c", base, v, N_CLS)], declined=declined)


def refinish(e, prev, shift):
    """msm_finish again on the state `prev` prepared, against the bases `shift` further on"""
    return Step("refinish of (%s), %d further" % (prev.what, shift), dict(kind=4, edwards=int(e), shift=shift), [("s",) + tuple((b + shift, s, n) for b, s, n in prev.outs[0][1:])])


def sizing(e):
    return win(e, N_UNI, U0, what="uniform sizing step, %d points" % N_UNI)


def skew1(e, base=0):
    return win(e, N_SKEW, S1, base=base, what="per-window, %d points under ONE distinct scalar" % N_SKEW)


def skew3(e, base=0):
    return win(e, N_SKEW, S3, base=base, what="per-window, %d points under three distinct scalars" % N_SKEW)


def tab_skew3(e):
    return tab(e, 16, 20_000, 0, S3, what="table c=16, 20,000 points under three distinct scalars")


def tab_skew1(e):
    return tab(e, 12, N, 0, S1, what="table c=12, 40,000 points under ONE distinct scalar")


def run_sequence(world, api, steps, poison):
    """ONE call; every step compared with the oracle; returns the results"""
    assert len(steps) <= api.MSM_SEQ_MAX_STEPS
    got = api.msm_sequence(world.bases, world.scalars, world.vals, [s.fields for s in steps], poison=poison)
    assert len(got) == len(steps)
    for i, (st, g) in enumerate(zip(steps, got)):
        what = "step %d of %d (%s)%s" % (i + 1, len(steps), st.what, ", accumulators poisoned" if poison and i else "")
        if st.refused:
            assert g["status"] == 1 and re.search(st.refused, g["error"]) and not g["accepted"], "%s: not refused with /%s/: status %d, '%s'" % (what, st.refused, g["status"], g["error"])
            assert g["points"] == [(bytes(96), False)] * 2, "%s: a refused step returned a point" % what
            continue
        assert g["status"] == 0, "%s: refused: %s" % (what, g["error"])
        if st.declined:
            assert not g["accepted"], "%s: accepted, but a value is out of range" % what
            continue
        assert g["accepted"], "%s: declined" % what
        for j, key in enumerate(st.outs):
            want = world.msm(key)
            xy, inf = g["points"][j]
            assert inf == want[1], "%s, point %d: infinity flag %s, the oracle says %s" % (what, j, inf, want[1])
            assert want[1] or xy == want[0], "%s, point %d: the sum differs from the oracle's" % (what, j)
    return got


# ---- 1. overflow then none, per-window ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("e", LAWS)
def test_per_window_msms_with_and_without_oversized_buckets_follow_each_other(world, api, e, poison):
    """stale overflow lists, ctrl[1] / ctrl[2] and ovf_slot; smaller c, nwin and bucket counts inside the buffers of larger ones"""
    run_sequence(world, api, [sizing(e), skew1(e), win(e, 1000, U0 + 300, base=777), win(e, 33, U0, base=5), skew3(e, base=64), win(e, 1 << 12, U0 + 9, base=N - (1 << 12))], poison)


# ---- 2. table mode across its two grouping paths ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("e", LAWS)
def test_table_msms_alternate_between_the_radix_sort_and_the_partition(world, api, e, poison):
    """between the partition (16-bit keys in keys_a, values through vals_a into vals_b) and the radix sort (32-bit keys, double-buffered) the same buffers change meaning;
    the skewed steps leave overflow lists behind for both.  (5,000 scalars under 16 bits take the PARTITION -- 80,000 pairs -- so 3,000 go first for the sort.)"""
    run_sequence(world, api, [sizing(e), tab(e, 16, 3_000, 0, U0), tab(e, 16, 5_000, 0, U0), tab(e, 18, 9_000, 0, U0),
                              tab(e, 18, 700, 300, U0 + 100, n2=500, off2=20_000, s2=U0 + 5_000),          # a pair at offsets, n1 + n2 far below the stride: back on the sort
                              tab_skew3(e), tab(e, 18, 9_000, 11, U0 + 10_000), tab(e, 15, 9_000, 0, U0 + 20_000), tab_skew1(e)], poison)


# ---- 3. the forms interleaved as a proof interleaves them ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("e", LAWS)
def test_class_sums_pairs_and_table_pairs_interleaved(world, api, e, poison):
    """the class sums carve their scratch from the bucket array of the MSM before; the flag word must have re-armed after the declined vector, with bucket MSMs in between"""
    run_sequence(world, api, [sizing(e), cls(e, V_A), win(e, 3_000, U0, base=100, n2=2_500, off2=4_000, s2=U0 + 3_000), cls(e, V_BAD, base=17, declined=True),
                              tab(e, 16, 2_000, 50, U0 + 6_000, n2=1_500, off2=30_000, s2=U0 + 8_000), cls(e, V_B, base=17), skew1(e), cls(e, V_C, base=N - N_CLS)], poison)


# ---- 4. two base arrays on one prepared state, with oversized buckets ------------------------------------------------------------------------------------------------------
def second_skew_window():
    return second(0, N_SKEW, 100, 15_000, S1, what="second bases per-window, %d points under ONE distinct scalar" % N_SKEW)


def second_skew_table():
    return second(16, 20_000, 7, 20_010, S3, what="second bases, table c=16, 20,000 points under three distinct scalars")


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("e", LAWS)
def test_msm_finish2_with_oversized_buckets_between_plain_msms(world, api, e, poison):
    """the tail kernel's ticket is taken and re-armed TWICE within one MSM (one launch per base array, one ticket word), into the second half of the buckets and of the
    overflow partials; each msm_finish2 is followed by a plain single MSM in the law of the run"""
    run_sequence(world, api, [sizing(e), second_skew_window(), win(e, 1000, U0 + 50, base=3), second_skew_table(), win(e, 2_000, U0, base=N - 2_000),
                              second(0, 5_000, 0, 123, U0 + 777), win(e, 33, U0 + 2, base=9)], poison)


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("e", LAWS)
@pytest.mark.parametrize("mode", ["per-window", "table"])
def test_msm_finish2_with_oversized_buckets_on_a_fresh_workspace(world, api, mode, e, poison):
    run_sequence(world, api, [second_skew_window() if mode == "per-window" else second_skew_table(), win(e, 1000, U0 + 50, base=3)], poison)


# ---- 5. one prepared state finished twice ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("e", LAWS)
def test_a_prepared_state_is_finished_again_against_other_bases(world, api, e, poison):
    """run_buckets documents it as allowed; skewed scalars, so the overflow list is live both times; per-window and table mode; an unrelated MSM behind each"""
    a, t = skew1(e), tab_skew3(e)
    run_sequence(world, api, [sizing(e), a, refinish(e, a, 12_345), win(e, 1 << 12, U0 + 4, base=1), t, refinish(e, t, 19_000), win(e, 1000, U0, base=2)], poison)


# ---- 6. mixed laws and the deferred list -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", POISON)
def test_both_laws_share_one_workspace_around_deferred_additions(world, api, poison):
    """64 equal bases under the scalar 3: the Weierstrass law defers 63 additions and replays them; the Edwards MSM behind it neither clears nor may read
    deferred_count[0]; its tail kernel takes tickets right after a Weierstrass one did.  The prover does not mix laws on a workspace; the interface allows it"""
    def equal(e):
        return win(e, RUN, T3, base=N, what="%d equal bases under the scalar 3" % RUN)
    run_sequence(world, api, [sizing(False), equal(False), win(True, 1 << 12, U0, base=10), win(False, 1000, U0 + 1, base=20), equal(False), skew1(True), equal(True), skew3(False)], poison)


# ---- 7. a refused step in the middle ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("e", LAWS)
def test_a_refused_step_leaves_the_workspace_fit_for_the_next_one(world, api, e, poison):
    """refused WHEN THEY RUN, not by the up-front argument checks: a per-window pair whose second range passes the end of the bases, a table step whose range exceeds the
    stride (msm_prepare_table's own refusal, after it has overwritten the plan's point count) and a refinish behind the refused step; each between a skewed and a uniform
    step.  Empty steps return infinity and disturb nothing"""
    t = tab_skew3(e)
    run_sequence(world, api, [sizing(e), skew1(e), win(e, 100, U0, n2=100, off2=NBASES - 50, s2=U0 + 100, refused="range exceeds the bases"), win(e, 1000, U0 + 7, base=40),
                              t, tab(e, 16, 300, NBASES - 299, U0, refused="msm_table: range exceeds the table"),
                              Step("refinish behind a refused step", dict(kind=4, edwards=int(e), shift=1), [], refused="no prepared state"), tab(e, 16, 3_000, 9, U0 + 11),
                              win(e, 0, U0, what="empty per-window step"), tab(e, 16, 0, 0, U0, what="empty table step"), win(e, 33, U0 + 1, base=3)], poison)


# ---- 8. the same step behind different histories ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("e", LAWS)
def test_a_step_gives_the_same_bytes_first_in_the_middle_and_last(world, api, e, poison):
    uni, skew = win(e, 5_000, U0 + 1_000, base=2_000, what="the fixed uniform step"), skew1(e)
    seqs = [[uni, tab_skew3(e), skew],                                           # uniform first, skewed last
            [skew, sizing(e), uni],                                              # skewed first, uniform last
            [sizing(e), uni, tab_skew1(e), skew, cls(e, V_A), win(e, 33, U0)]]    # both in the middle
    got = [run_sequence(world, api, s, poison) for s in seqs]
    for fixed in (uni, skew):
        pts = [g[s.index(fixed)]["points"][0] for s, g in zip(seqs, got)]
        assert pts[0] == pts[1] == pts[2] == world.msm(fixed.outs[0]), "%s depends on what ran before it" % fixed.what


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_bad_sequences_are_refused_before_anything_is_allocated(world, api):
    """null arguments, too many steps, a range outside a blob and bad window bits: a non-zero return with a message in zkaes_last_error, and no device memory taken"""
    L = api.lib()
    good = [sizing(True).fields, tab(False, 12, 700, 10, U0).fields]
    api.msm_sequence(world.bases, world.scalars, world.vals, good)                  # warm the runtime's own pools before the first reading
    free0, _ = api.mem_info()

    def refused(steps, pattern):
        with pytest.raises(api.ZkAesError, match=pattern):
            api.msm_sequence(world.bases, world.scalars, world.vals, steps)

    nsc = len(world.scalars) // 32
    for _ in range(3):
        refused([], "1..32 steps")
        refused(good * 17, "1..32 steps")
        refused([win(True, 10, nsc - 9).fields], "scalar range outside the scalars")
        refused([win(True, 10, 0, n2=5, off2=3, s2=nsc - 4).fields], "scalar range outside the scalars")
        refused([tab(False, 16, 1, 0, nsc).fields], "scalar range outside the scalars")
        refused([dict(kind=3, edwards=1, n1=N_CLS, scal1=len(world.vals) - N_CLS + 1)], "value range outside the class values")
        for bits in (0, 1, 23):
            refused([tab(True, bits, 10, 0, U0).fields], "window bits")
        refused([second(23, 10, 0, 5, U0).fields], "window bits")
        refused([dict(kind=5)], "unknown step kind")
        refused([dict(kind=0, reserved=1)], "unknown step kind")
        refused([dict(kind=0, n1=1, off1=(1 << 26) + 1)], "2\\^26")
        refused([dict(kind=2, edwards=0, n1=10)], "Edwards law")
        refused([dict(kind=4, edwards=1)], "needs a preparing step")
        refused([cls(True, V_A).fields, dict(kind=4, edwards=1)], "needs a preparing step")
        refused([tab(True, c, 10, 0, U0).fields for c in range(4, 13)], "distinct window bits")
        # null pointers, straight at the C entry point
        st = (api.MsmStep * 1)(api.MsmStep(**good[0]))
        out, inf, ok, status, err = C.create_string_buffer(192), (C.c_int * 2)(), (C.c_int * 1)(), (C.c_int * 1)(), C.create_string_buffer(api.MSM_SEQ_ERR_BYTES)
        b, v = world.bases.ctypes.data_as(C.c_void_p), world.vals.ctypes.data_as(C.c_void_p)
        nb, nv = C.c_size_t(NBASES), C.c_size_t(len(world.vals))
        for args in ((None, nb, world.scalars, C.c_size_t(nsc), v, nv, st, C.c_size_t(1), 0, out, inf, ok, status, err),
                     (b, nb, None, C.c_size_t(nsc), v, nv, st, C.c_size_t(1), 0, out, inf, ok, status, err),
                     (b, nb, world.scalars, C.c_size_t(nsc), None, nv, st, C.c_size_t(1), 0, out, inf, ok, status, err),
                     (b, nb, world.scalars, C.c_size_t(nsc), v, nv, None, C.c_size_t(1), 0, out, inf, ok, status, err),
                     (b, nb, world.scalars, C.c_size_t(nsc), v, nv, st, C.c_size_t(1), 0, None, inf, ok, status, err),
                     (b, nb, world.scalars, C.c_size_t(nsc), v, nv, st, C.c_size_t(1), 0, out, None, ok, status, err),
                     (b, nb, world.scalars, C.c_size_t(nsc), v, nv, st, C.c_size_t(1), 0, out, inf, None, status, err),
                     (b, nb, world.scalars, C.c_size_t(nsc), v, nv, st, C.c_size_t(1), 0, out, inf, ok, None, err),
                     (b, nb, world.scalars, C.c_size_t(nsc), v, nv, st, C.c_size_t(1), 0, out, inf, ok, status, None)):
            assert L.zkaes_msm_sequence(*args) != 0 and b"null" in L.zkaes_last_error()
        assert L.zkaes_msm_sequence(b, C.c_size_t(0), world.scalars, C.c_size_t(nsc), v, nv, st, C.c_size_t(1), 0, out, inf, ok, status, err) != 0 and b"nbases" in L.zkaes_last_error()
    free1, _ = api.mem_info()
    assert free0 - free1 < 16 << 20, "a refused sequence took device memory: %d bytes" % (free0 - free1)
    run_sequence(world, api, [sizing(True), tab(False, 12, 700, 10, U0)], False)      # the good path afterwards
