"""Big-integer restatement of the MSM's two window plans and of its signed-digit recoding (csrc/kernels_msm.hip: msm_prepare, table_layout, k_digits, k_digits_table,
part_digits).  TEST INFRASTRUCTURE: it exists to CONSTRUCT and CERTIFY the scalars that reach the recoding's edges -- tests/test_msm_model.py checks it on the CPU,
tests/test_gpu_msm_forms.py feeds the certified scalars to the kernels.  The expected sums of the GPU tests do not come from here: they come from the CPU oracle."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "aes_zero_knowledge_proof_circuit_amd", "csrc", "kernels_msm.hip")

R = 0x12ab655e9a2ca55660b44d1e5c37b00159aa76fed00000010a11800000000001       # BLS12-377 scalar field
DIGIT_BITS = 254                                                              # Fr::BITS + 1: one bit above the 253-bit modulus for the recoding carry


def constants():
    """the constants of kernels_msm.hip that the GPU tests' shapes are derived from, READ from the source: a re-tuned constant moves its cases with it"""
    text = open(SOURCE).read()

    def one(pattern, what):
        m = re.search(pattern, text)
        assert m, "%s not found in kernels_msm.hip" % what
        return int(m.group(1))

    c = {name: one(r"\b%s = (\d+)\b" % name, name) for name in ("CLS_CHUNK", "MAX_WSUMS", "RQ_THREADS", "BUCKET_CAP_TABLE", "PART_FINE_BITS", "PART_WBITS", "PART_NBIN_MAX")}
    assert re.search(r"\bRQ_QUADS = RQ_THREADS / 4\b", text), "RQ_QUADS is no longer RQ_THREADS / 4"
    c["RQ_QUADS"] = c["RQ_THREADS"] // 4
    # msm_prepare_table: ... && nwin <= PART_MAXW && pairs >= ((size_t)1 << 16)) partition_buckets(...)
    c["PART_MIN_PAIRS"] = 1 << one(r"nwin <= PART_MAXW && pairs >= \(\(size_t\)1 << (\d+)\)\) \{\s*partition_buckets", "the partition threshold")
    return c


class Plan:
    """windows as (offset, width) pairs, lowest first"""

    def __init__(self, name, windows):
        self.name, self.windows = name, list(windows)
        self.nwin = len(self.windows)

    def offset(self, j):
        return self.windows[j][0]

    def width(self, j):
        return self.windows[j][1]

    def half(self, j):
        return 1 << (self.windows[j][1] - 1)

    def from_fields(self, fields):
        return sum(f << self.offset(j) for j, f in enumerate(fields))

    def __repr__(self):
        return self.name


def window_bits_for(n):
    """msm_prepare: c = clamp(ceil(lg n) - 2, 7, 17)"""
    lg = 0
    while (1 << lg) < n:
        lg += 1
    return min(max(lg - 2, 7), 17)


def per_window_plan(n):
    """the plan msm_prepare picks for n points: nwin = ceil(254 / c) windows of c bits, one bucket set each"""
    c = window_bits_for(n)
    nwin = (DIGIT_BITS + c - 1) // c
    return Plan("per-window c=%d" % c, [(j * c, c) for j in range(nwin)])


def table_layout(c, total_bits=DIGIT_BITS):
    """TableLayout: (nwin, c_hi, n_hi) -- the total spread as evenly as possible, windows j < n_hi are c_hi bits wide, the others c_hi - 1"""
    nwin = (total_bits + c - 1) // c
    base, rem = divmod(total_bits, nwin)
    return nwin, base + (1 if rem else 0), rem if rem else nwin


def table_plan(c):
    nwin, c_hi, n_hi = table_layout(c)
    windows, off = [], 0
    for j in range(nwin):
        w = c_hi if j < n_hi else c_hi - 1
        windows.append((off, w))
        off += w
    assert off == DIGIT_BITS
    return Plan("table c=%d" % c, windows)


def partition_accepts(c, pairs, k=None):
    """msm_prepare_table's choice between the two-level partition and digits + radix sort"""
    k = k or constants()
    nwin, c_hi, _ = table_layout(c)
    b = c_hi - 1
    return b > k["PART_FINE_BITS"] and (1 << (b - k["PART_FINE_BITS"])) <= k["PART_NBIN_MAX"] and nwin <= (1 << k["PART_WBITS"]) and pairs >= k["PART_MIN_PAIRS"]


def recode(s, plan, recode_at_half=False):
    """per window: (signed digit, skip, carry out), as k_digits / k_digits_table / part_digits compute them; the last carry must be 0 for the digits to represent s.
    recode_at_half: the variant that also recodes a digit of exactly half (v >= half), for the proof that it is the same recoding"""
    out, carry = [], 0
    for off, w in plan.windows:
        v = ((s >> off) & ((1 << w) - 1)) + carry
        carry, neg = 0, False
        if v > (1 << (w - 1)) or (recode_at_half and v == (1 << (w - 1))):
            v, neg, carry = (1 << w) - v, True, 1
        out.append((-v if neg else v, v == 0, carry))
    return out


def digits_value(digits, plan):
    return sum(d << plan.offset(j) for j, (d, _, _) in enumerate(digits))


def _fit(fields, plan):
    """clear high windows until the scalar is below r"""
    fields = list(fields)
    j = plan.nwin - 1
    while plan.from_fields(fields) >= R:
        fields[j] = 0
        j -= 1
    return plan.from_fields(fields)


def edge_scalars(plan):
    """name -> scalar < r, every one of them built to reach one edge of the recoding under `plan` (tests/test_msm_model.py certifies that each does):
      half            every window field = half: the largest digit that stays positive, no carry anywhere
      half_plus_one   every window field = half + 1: the smallest value that recodes (digit -(half - 1) + carry); the windows above see half + 2
      half_then_carry field 0 = half + 1, the others = half: every window above the first reaches half + 1 only THROUGH the carry
      all_ones        2^252 - 1: every window but the first becomes 2^c after the carry -> digit 0 with SKIP set and a carry still going out
      carry_to_top    all ones below the top window, the top field 0: the top digit is 1 and exists only because of the carry
      pow2_K, pow2m1_K  2^K and 2^K - 1 at every window boundary and at every 32-bit limb boundary that a window straddles"""
    top = plan.nwin - 1
    e = {}
    e["half"] = _fit([plan.half(j) for j in range(plan.nwin)], plan)
    e["half_plus_one"] = _fit([plan.half(j) + 1 for j in range(plan.nwin)], plan)
    e["half_then_carry"] = _fit([plan.half(j) + (1 if j == 0 else 0) for j in range(plan.nwin)], plan)
    e["all_ones"] = (1 << 252) - 1
    e["carry_to_top"] = (1 << plan.offset(top)) - 1
    ks = set(plan.offset(j) for j in range(1, plan.nwin))
    for limb in range(1, 8):
        if any(off < 32 * limb < off + w for off, w in plan.windows):
            ks.add(32 * limb)
    for k in sorted(ks):
        if k <= 252:
            e["pow2_%d" % k] = 1 << k
            e["pow2m1_%d" % k] = (1 << k) - 1
    assert all(0 <= v < R for v in e.values())
    return e


# the sizes and window bits the GPU tests run (tests/test_gpu_msm_forms.py takes them from here; tests/test_msm_model.py certifies the edge scalars of every plan they give)
PAIR_TOTALS = (2, 512, 513, 1024, 1025, (1 << 14) + 1)        # n1 + n2 of the two-vector cases: c = 7 | 7 | 8 | 8 | 9 | 13
SECOND_BASES_SIZES = (512, 513, 1025)                       # 2 x 37 window sums (sequential), 2 x 32 = MAX_WSUMS exactly, 2 x 29
TABLE_BITS = (20, 17, 15, 12)                               # partition (19 and 16 bucket bits), 17 windows (radix sort at any size), a small plan


def gpu_test_plans():
    plans = {}
    for n in PAIR_TOTALS + SECOND_BASES_SIZES:
        p = per_window_plan(n)
        plans[p.name] = p
    for c in TABLE_BITS:
        p = table_plan(c)
        plans[p.name] = p
    return list(plans.values())
