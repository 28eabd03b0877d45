"""GPU: Fp2 and the Fp6 / Fp12 tower operation by operation, as compiled for the device (vsp_selftest_tower), and the lane-pair Fp2 of
the G2 kernels (vsp_selftest_fp2_lanes), on the case list of tower_cases.py -- zero coefficients, p - 1, subfield elements,
c0 = +-c1, sums that wrap past p -- against the oracle's integers.  test_pairing_cpu.py runs the same list through the g++ build of the
same headers, so a failure here means the device code differs from that build.  Exact equality of canonical words everywhere."""
import ctypes as C

import numpy as np
import pytest

import tower_cases as tc

pytestmark = pytest.mark.gpu

ERR_ARG = -1


def ptr(x):
    return x.ctypes.data_as(C.c_void_p)


def run_tower(ctx, level, op, a, b):
    assert a.shape == b.shape and a.shape[1] == 6 * level
    out = np.zeros_like(a)
    ctx.check(ctx.lib.vsp_selftest_tower(ctx.h, level, op, ptr(a), ptr(b), ptr(out), a.shape[0]))
    return out


def run_lanes(ctx, form, op, ops):
    a, b, c, d = ops
    p, q = np.zeros_like(a), np.zeros_like(a)
    ctx.check(ctx.lib.vsp_selftest_fp2_lanes(ctx.h, form, op, ptr(a), ptr(b), ptr(c), ptr(d), ptr(p), ptr(q), a.shape[0]))
    return p, q


def bad_rows(got, want):
    return np.flatnonzero((got != want).any(axis=1))[:8].tolist()


def launch_sizes(cases):
    """the sizes 65, 127 and 130 for a list of `cases` rows: the list is repeated up to the size; a list longer than the size goes in
    one launch of the next length that leaves the same lanes in the last 64-lane block (1, 63 and 2)"""
    for n in tc.PAD_SIZES:
        while n < cases:
            n += 64
        yield n


@pytest.fixture(scope="module")
def cases():
    return tc.tower_cases()


@pytest.fixture(scope="module")
def lanes():
    return tc.lane_cases()


@pytest.mark.parametrize("level", [2, 6, 12])
def test_every_operation_of_a_level_against_the_oracle(ctx, cases, level):
    for (lv, op), (a, b, want) in sorted(cases.items()):
        if lv != level:
            continue
        for n in launch_sizes(a.shape[0]):
            assert n % 64 in (1, 63, 2) and n > 64
            got = run_tower(ctx, level, op, tc.pad(a, n), tc.pad(b, n))
            assert not bad_rows(got, tc.pad(want, n)), (level, op, n, bad_rows(got, tc.pad(want, n)))


@pytest.mark.parametrize("form", [0, 1])
def test_lane_pair_operations_one_op_per_launch_and_mixed(ctx, lanes, form):
    """each op of the form over the whole Fp2 list, then op -1: element i runs op i mod K, so the pairs of one wave branch apart.
    p and q are asserted separately (q is zero for every op but mul_pair)"""
    ops, want = lanes
    n = ops[0].shape[0]
    assert n % 2 == 1 and n % 32 != 0
    for op in list(range(tc.LANE_OPS[form])) + [-1]:
        p, q = run_lanes(ctx, form, op, ops)
        wp, wq = want[form, op]
        assert not bad_rows(p, wp), (form, op, "p", bad_rows(p, wp))
        assert not bad_rows(q, wq), (form, op, "q", bad_rows(q, wq))


def test_cross_checks_that_need_no_oracle(ctx, cases, lanes):
    one = {lv: np.zeros(6 * lv, np.uint64) for lv in (2, 6, 12)}
    for lv in one:
        one[lv][0] = 1
    for lv in (2, 6, 12):
        a = cases[lv, 2][0]                                         # the operands of the inverse: every value of the level
        sq = run_tower(ctx, lv, 0, a, a)
        if lv == 6:                                                 # Fp6 has no square of its own: the Fp12 square of the embedded value
            emb = np.concatenate([a, np.zeros_like(a)], axis=1)
            assert np.array_equal(run_tower(ctx, 12, 1, emb, emb), np.concatenate([sq, np.zeros_like(sq)], axis=1))
        else:
            assert np.array_equal(run_tower(ctx, lv, 1, a, a), sq)
        prod = run_tower(ctx, lv, 0, a, run_tower(ctx, lv, 2, a, a))
        nonzero = a.any(axis=1)
        assert nonzero.any() and not nonzero.all()
        assert (prod[nonzero] == one[lv]).all() and not prod[~nonzero].any()
    a = cases[12, 4][0]
    f1 = run_tower(ctx, 12, 4, a, a)
    assert np.array_equal(run_tower(ctx, 12, 4, f1, f1), run_tower(ctx, 12, 5, a, a))
    # the lane-pair product, the 28-bit pair product and the one-lane product on the same operands
    ops, _ = lanes
    t = run_tower(ctx, 2, 0, ops[0], ops[1])
    l, _ = run_lanes(ctx, 0, 0, ops)
    assert np.array_equal(l, t)
    for op in (0, 1):
        assert np.array_equal(run_lanes(ctx, 1, op, ops)[0], l)


def test_error_paths_leave_the_context_working(ctx, cases):
    a, b, want = cases[2, 0]
    a, b, want = a[:65], b[:65], want[:65]
    out = np.zeros_like(a)
    opt = lambda x: ptr(x) if x is not None else None
    tower = lambda level, op, x=a, y=b, o=out: ctx.lib.vsp_selftest_tower(ctx.h, level, op, opt(x), opt(y), opt(o), 65)
    for level, op in ((0, 0), (3, 0), (4, 0), (24, 0), (-2, 0), (2, -1), (2, 14), (6, 5), (6, 6), (6, 9), (12, 13), (12, -1)):
        assert tower(level, op) == ERR_ARG, (level, op)
    assert tower(2, 0, x=None) == ERR_ARG and tower(2, 0, y=None) == ERR_ARG and tower(2, 0, o=None) == ERR_ARG
    assert ctx.lib.vsp_selftest_tower(None, 2, 0, ptr(a), ptr(b), ptr(out), 65) == ERR_ARG
    assert "selftest" in ctx.last_error()
    q = np.zeros_like(a)
    bufs = [a, b, a, b, out, q]
    lanes_call = lambda form, op, args: ctx.lib.vsp_selftest_fp2_lanes(ctx.h, form, op, *[opt(x) for x in args], 65)
    for form, op in ((2, 0), (-1, 0), (0, 10), (0, -2), (1, 5), (1, 9)):
        assert lanes_call(form, op, bufs) == ERR_ARG, (form, op)
    for k in range(6):
        assert lanes_call(0, 0, bufs[:k] + [None] + bufs[k + 1:]) == ERR_ARG, k
    assert not out.any() and not q.any()                            # a refused call writes nothing
    assert np.array_equal(run_tower(ctx, 2, 0, a, b), want)
    p, _ = run_lanes(ctx, 0, 0, (a, b, a, b))
    assert np.array_equal(p, want)
