"""GPU parity tests of the field and curve arithmetic's DEVICE branches (csrc/ff.cuh 32-bit CIOS, ff28.cuh / ff29.cuh v_sad_u32 and __umulhi forms, the opaque hot-loop bias,
te28.cuh's four-lanes-per-point forms): ONE operation per launch through zkaes_arith_probe, on the operand lists of tests/arith_model.py, against its big-integer model.

Field operations are compared by BYTE EQUALITY of the raw limbs (a Montgomery product of integers is one determined integer, also for lazy operands); the group law as points
against tools/curve_math.py, plus byte equality between the device's own paths where the header promises it.  tests/test_arith_model.py has validated the same model and the
same operands against the host branch, so a failure here names an operation, an operand and the branch."""
import pytest

import arith_model as am

pytestmark = pytest.mark.gpu
OPS = sorted(n for n in am.ARITH_OPS if n != am.HOT)


def run(api, name, ins):
    return am.unpack(api.arith_probe(name, am.pack(ins)), am.ARITH_OPS[name][2])


@pytest.mark.parametrize("name", OPS)
def test_device_branch_equals_the_model(api, name):
    ins = am.cases(name)
    am.check(name, ins, run(api, name, ins))


def test_biased_product_equals_the_plain_one_limb_for_limb(api):
    """mul_biased (columns started at the opaque SGPR bias) against operator* on the same operands, te_madd_hot's limb bounds included"""
    ins = am.cases("fq377x28.mul_biased")
    assert run(api, "fq377x28.mul_biased", ins) == run(api, "fq377x28.mul", ins)


@pytest.mark.parametrize("quad, whole", [("te377.te_add_quad", "te377.te_add"), ("te377.te_dbl_quad", "te377.te_dbl")])
def test_quad_forms_give_the_bytes_of_the_whole_lane_forms(api, quad, whole):
    """te28.cuh promises "same results".  The case count is no multiple of 16, so the last wave has idle quads beside live ones (the callers run the quad forms under
    `if (active)`); one case and seventeen cases put the boundary elsewhere."""
    ins = am.cases(quad)
    assert len(ins) % 16 and len(ins) > 64
    want = run(api, whole, ins)
    assert run(api, quad, ins) == want
    for n in (1, 3, 17):
        assert run(api, quad, ins[:n]) == want[:n]


def test_hot_addition_chains(api):
    """seven te_madd_hot in a row with mixed signs of the current and of the next digit, checked as points after every step and for the record left in n; for a positive
    digit the same bytes as te_madd of the same record (every factor is the same integer in another limb layout)"""
    prev = None
    for step in range(7):
        ins = am.hot_step_cases(step, prev)
        prev = run(api, am.HOT, ins)
        am.hot_step_check(step, prev)
        plain = [(c, x) for c, x in enumerate(am.hot_as_madd(ins)) if x is not None]
        madd = run(api, "te377.te_madd", [x for _, x in plain])
        assert plain and all(prev[c][:56] == m for (c, _), m in zip(plain, madd)), "te_madd_hot differs from te_madd at step %d" % step
    signs = {(negs[0], negs[1]) for _, _, negs in am.HOT_CHAINS}
    assert signs == {(False, False), (False, True), (True, False), (True, True)}


def test_a_full_launch_of_65536_cases(api):
    """the largest launch the entry point accepts: 1024 workgroups, every case checked"""
    base = am.cases("fr377x29.sub_lazy2")
    ins = (base * (65536 // len(base) + 1))[:65536]
    out = run(api, "fr377x29.sub_lazy2", ins)
    want = am.expected("fr377x29.sub_lazy2")
    assert all(out[i] == want[i % len(base)] for i in range(65536))
