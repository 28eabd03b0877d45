"""CPU: the lean form of the generated G1 accumulation routine (tools/gen_accum28_asm.py -> accum28_asm_gfx950.h).

The routine no longer carries P = x ZZ + 32p - X and R = y ZZZ + 32p - Y to tight limbs, tests for infinity and for equal x on limb 0 only
(the full tests sit in cold blocks behind the loop's back branch) and starts every product's column accumulator from a zero SGPR pair.
None of that may change a result bit or let a column accumulator wrap.  Checked here, without a GPU:

 (a) an exact limb model of the loop body with P and R LOOSE -- the limb bounds are the largest the subtraction can produce with the
     generator's own K32_L1 / K8_L1 / K8_L4 limbs, the top limb included: every column of every product and square that reads a loose block
     stays below 2^64, the doubled operand of a square fits 32 bits, and the invariants of fp28.h hold at loop exit; the same model, run on
     limb vectors that ARE those maxima and on accumulator states at the invariants' worst case, gives the outputs of the model with the
     carry passes, bit for bit;
 (b) the generated stream in the interpreter of tests/test_accum28_asm.py on the inputs that separate the limb-0 tests from the full ones:
     a finite row whose x and y both have limb 0 zero, an accumulator whose ZZ has limb 0 zero, a PP whose limb 0 is 0 or p_0 while PP is
     neither 0 nor p -- beside real doublings, cancellations, rows at infinity, ordinary lanes and lanes outside EXEC;
 (c) the instruction count of one iteration on the common path.

How the special inputs are made.  A random search cannot reach them in seconds (2^-27 per lane for PP, 2^-28 for ZZ, 2^-56 for a row), so
they are SOLVED for and then confirmed by the exact model: with the accumulator holding its first point (ZZ = ZZZ = one) the next addition has
PP = (x2 - x1)^2 / R' and ZZ' = PP mod p, so a wanted PP or ZZ' fixes x2 = x1 + sqrt(.); candidates are tried until x2 is the abscissa of a
point of y^2 = x^3 + 4 and the model shows the wanted limb.  (Such a point lies on the curve, not necessarily in the subgroup of order r:
the addition formulas do not ask.)  The row with limb 0 zero in x AND y is a point of y^2 = x^3 + b for another b: the mixed addition never
reads b, and the expected sum is the chord formula of the oracle, which does not read it either."""
import random

import numpy as np

import bls12_381 as o
import test_accum28_asm as ta
import test_fp28_bounds as fb

gen = ta.gen
P, N, W, MASK, RP, LANES = ta.P, ta.N, ta.W, ta.MASK, ta.RP, ta.LANES
RINV = pow(RP, -1, P)
K32, K8L1, K8L4 = gen.K32_L1, gen.K8_L1, gen.K8_L4
ONE = gen.ONE28

# the parent's loop (commit 6fef17f, counted as bench.py's roofline_valu counts it: from .Lvsp_acc28_loop to the back branch, the first-point
# block aside) and what this form removes: 2 x 39 (carry passes) + 20 (infinity tests) + 36 (equal-x test) + 18 (accumulator zeroing)
PARENT_MAD, PARENT_VALU_OTHER, REMOVED = 3544, 1050, 152


def test_the_generators_constants_are_the_headers():
    assert K32 == fb.K["FP28_K32_L1"] and K8L1 == fb.K["FP28_K8_L1"] and K8L4 == fb.K["FP28_K8_L4"]
    assert gen.P28 == fb.PL and ONE == fb.K["FP28_ONE"] and gen.INV28 == fb.INV28


# ------------------------------------------------------------------------------------------------ (a) the limb model
def sq_loose(a):
    """the generator's square (Emit.sqr + product(sqr_of=)): a2 = 2a limb by limb in 32 bits, off-diagonal products once against a2.
    Unlike fb.sq28 it takes a LOOSE a; every column is checked, and the result must be the product a * a"""
    a2 = [2 * t for t in a]
    fb.need(all(t < 1 << 32 for t in a2), "the doubled operand of a square wraps a 32-bit limb")
    m, r, acc, worst = [0] * N, [0] * N, 0, 0
    for k in range(2 * N - 1):
        for i in range(max(0, k - N + 1), min(k, N - 1) + 1):
            if i < k - i:
                acc += a[i] * a2[k - i]
            elif i == k - i:
                acc += a[i] * a[i]
        for i in (range(0, k) if k < N else range(k - N + 1, N)):
            acc += m[i] * fb.PL[k - i]
        if k < N:
            m[k] = (((acc & 0xFFFFFFFF) * fb.INV28) & 0xFFFFFFFF) & MASK
            acc += m[k] * fb.PL[0]
        else:
            r[k - N] = acc & MASK
        fb.need(acc < 1 << 64, "column %d of the square overflows" % k)
        worst = max(worst, acc)
        acc >>= W
    fb.need(acc < 1 << 32, "top limb of the square overflows")
    r[N - 1] = acc
    fb.need(r == fb.mm28(a, a), "the square differs from the product a * a")
    return r, worst


def lean_madd28(acc, q, negate):
    """the loop body as the routine now runs it: fb.madd28 without the carry passes of P and R"""
    qx, qy = q
    qyn = fb.neg28(K8L1, qy) if negate else qy
    X, Y, ZZ, ZZZ = acc
    Pd = fb.sub28(fb.mm28(qx, ZZ), K32, X)                  # loose
    R = fb.sub28(fb.mm28(qyn, ZZZ), K32, Y)                 # loose
    PP, _ = sq_loose(Pd)
    if fb.is_zero_product(PP, 2):
        return acc, False
    PPP, Q = fb.mm28(Pd, PP), fb.mm28(X, PP)
    RR, _ = sq_loose(R)
    X3 = fb.norm28(fb.sub28(RR, K8L4, fb.lin(PPP, 1, Q, 2)))
    Y3 = fb.mm28(R, fb.sub28(Q, K32, X3), fb.neg28(K32, Y), PPP)
    return (X3, Y3, fb.mm28(ZZ, PP), fb.mm28(ZZZ, PPP)), True


def test_limb_model_worst_case_columns_and_exit_invariants():
    """value bound and limb bound per position through the loop body, the loose blocks at the LARGEST limbs a + K32_L1 - b can have
    (a limb of a at its maximum, the limb of b zero).  fb.b_mul sums a column from these maxima (a square's column total is the product's)
    and refuses 2^64; fb.b_sub refuses a borrow and a 32-bit wrap."""
    B = fb.B
    one = B(1, [1] * N)
    X, Y, ZZ, ZZZ = B.tight(9.5 * P), B.tight(8 * P + 1), B.tight(1.1 * P), B.tight(1.1 * P)
    qx = B.tight(P)
    for qy in (B.tight(P), fb.b_sub(one, "FP28_K8_L1", B.tight(P))):
        U2, S2 = fb.b_mul(qx, ZZ), fb.b_mul(qy, ZZZ)
        Pd = fb.b_sub(U2, "FP28_K32_L1", X)                                  # NO carry pass
        R = fb.b_sub(S2, "FP28_K32_L1", Y)                                   # NO carry pass
        for blk in (Pd, R):
            assert blk.l[:N - 1] == [(1 << W) + K32[i] for i in range(N - 1)]             # the maxima named above, exclusive
            assert max(blk.l[:N - 1]) <= 3 << 28                                          # 1.5 * 2^29
            assert blk.l[N - 1] > K32[N - 1] and blk.v < 33.6 * P
            fb.b_lin(blk, 2, one, 0)                                                      # 2P, 2R fit 32 bits
        PP = fb.b_mul(Pd, Pd); assert PP.v < 1.45 * P                        # the test against {0, p} stays exhaustive
        RR = fb.b_mul(R, R); assert RR.v < 1.45 * P
        PPP, Q = fb.b_mul(Pd, PP), fb.b_mul(X, PP)
        s = fb.b_lin(PPP, 1, Q, 2)
        X3 = fb.b_norm(fb.b_sub(RR, "FP28_K8_L4", s)); assert X3.v < 9.5 * P
        D = fb.b_sub(Q, "FP28_K32_L1", X3); assert max(D.l[:-1]) <= 3 << 28
        nY = fb.b_sub(one, "FP28_K32_L1", Y); assert max(nY.l[:-1]) <= 1 << 29
        Y3 = fb.b_mul(R, D, nY, PPP); assert Y3.v < 1.5 * P                  # R loose AND D loose: the widest columns of the loop
        ZZ3, ZZZ3 = fb.b_mul(ZZ, PP), fb.b_mul(ZZZ, PPP)
        # fp28.h at loop exit: X < 9.5p, Y < 1.5p (8p in the first-point case: the copy), ZZ, ZZZ < 1.1p, all tight (product outputs, X3 carried)
        assert ZZ3.v < 1.1 * P and ZZZ3.v < 1.1 * P and X3.v <= X.v and Y3.v <= Y.v
        assert all(b.l[:-1] == [1 << W] * (N - 1) for b in (X3, Y3, ZZ3, ZZZ3))


def test_limb_model_exact_at_the_maximal_loose_limbs():
    """the exact schedules on limb vectors that ARE the maxima: every limb of a product output 2^28 - 1 (top limb: the largest a value below
    1.45p leaves), the subtrahend zero.  The columns are the true worst case, not an estimate of it."""
    top = lambda mult: int(mult * 1000) * P // 1000 >> (W * (N - 1))
    out_max = [MASK] * (N - 1) + [top(1.45)]
    zero = [0] * N
    loose_max = fb.sub28(out_max, K32, zero)
    assert loose_max == [MASK + K32[i] for i in range(N - 1)] + [top(1.45) + K32[N - 1]]
    r, worst = sq_loose(loose_max)
    assert worst < 1 << 64 and worst > 1 << 62                                # close to the bound: the model is not vacuous
    fb.mm28(loose_max, out_max)                                                # P PP: loose x tight
    fb.mm28(loose_max, loose_max, fb.neg28(K32, zero), out_max)                # R (Q + 32p - X3) + (32p - Y) PPP with R and the difference loose


def _lift(x, cap_mult):
    kmax = int(cap_mult * 1000) * P // 1000
    return x + ((kmax - x) // P) * P


def test_lean_body_is_bit_identical_to_the_body_with_carry_passes():
    rng = random.Random(21)
    pts = fb.rand_points_g1(rng, 10)
    base = o.G1.mul(o.G1.gen, 0xFACADE)
    for pt in pts:
        z = rng.randrange(1, P)
        zz, zzz = z * z % P, z * z * z % P
        X, Y = base[0] * zz % P, base[1] * zzz % P
        states = [(fb.tight(_lift(X * RP % P, 9.5)), fb.tight(_lift(Y * RP % P, 8.0)), fb.tight(_lift(zz * RP % P, 1.1)), fb.tight(_lift(zzz * RP % P, 1.1))),
                  (fb.to28(X), fb.to28(Y), fb.to28(zz), fb.to28(zzz))]
        for acc in states:
            for negate in (False, True):
                q = (fb.to28(pt[0]), fb.to28(pt[1]))
                lean, ok = lean_madd28(acc, q, negate)
                assert ok and (lean, ok) == fb.madd28(acc, q, negate)
                assert fb.acc_affine(lean) == o.G1.add(base, o.G1.neg(pt) if negate else pt)
                assert fb.val(lean[0]) < 9.5 * P and fb.val(lean[1]) < 1.5 * P and fb.val(lean[2]) < 1.1 * P and fb.val(lean[3]) < 1.1 * P
                assert all(x <= MASK for c in lean for x in c[:-1])
    single, _ = fb.madd28(None, (fb.to28(pts[0][0]), fb.to28(pts[0][1])), False)
    for negate in (False, True):                                                # equal x: handed back untouched, as before
        assert lean_madd28(single, (fb.to28(pts[0][0]), fb.to28(pts[0][1])), negate) == (single, False)


# ------------------------------------------------------------------------------------------------ (b) the generated stream
class Visits(dict):
    """the interpreter's label table, counting the branches TAKEN to each label"""

    def __init__(self, d):
        super().__init__(d)
        self.taken = {}

    def __getitem__(self, k):
        self.taken[k] = self.taken.get(k, 0) + 1
        return super().__getitem__(k)


def run(table_pts, ranges, entries, exec_mask=(1 << LANES) - 1):
    m = ta.Machine(gen.gen_body())
    m.labels = Visits(m.labels)
    m.mem[ta.TABLE_BASE] = np.array([w for pt in table_pts for w in ta.mont_point(pt)], dtype=ta.U32)
    m.mem[ta.SORTED_BASE] = np.array(entries, dtype=ta.U32)
    m.s[36], m.s[37] = ta.TABLE_BASE & 0xFFFFFFFF, ta.TABLE_BASE >> 32
    m.s[38], m.s[39] = ta.SORTED_BASE & 0xFFFFFFFF, ta.SORTED_BASE >> 32
    m.s[50], m.s[51] = 0xDEADBEEF, 0x12345678                                    # the routine sets its own zero pair
    rng = np.random.default_rng(6)
    m.v[:] = rng.integers(0, 1 << 32, size=m.v.shape, dtype=np.uint64).astype(ta.U32)
    for lane, (a, b) in enumerate(ranges):
        m.v[157, lane], m.v[158, lane] = a, b
    before = m.v.copy()
    m.exec = exec_mask
    m.run()
    assert m.exec == exec_mask and max(m.written) < gen.NVGPR <= 168
    return m, before


def check_lane(m, lane, want):
    X, Y, ZZ, ZZZ = ta.lane_result(m, lane)
    zz, zzz = ta.val(ZZ) % P, ta.val(ZZZ) % P
    assert zz and pow(zz * RINV, 3, P) == pow(zzz * RINV, 2, P)
    assert (ta.val(X) * pow(zz, -1, P) % P, ta.val(Y) * pow(zzz, -1, P) % P) == want, lane
    for limbs, bound in ((X, 9.5), (Y, 8.0), (ZZ, 1.1), (ZZZ, 1.1)):
        assert all(x <= MASK for x in limbs[:-1]) and ta.val(limbs) < bound * P


def mont(pt):
    return fb.tight(pt[0] * RP % P), fb.tight(pt[1] * RP % P)


def on_curve_with_x(xm):
    """the point whose Montgomery abscissa is xm, if xm / R' is the abscissa of a point of y^2 = x^3 + 4"""
    x = xm * RINV % P
    y = o.fp_sqrt((x * x * x + 4) % P)
    return None if y is None else (x, y)


def second_point_for(p1, wanted_pp_mod_p):
    """p2 with (x2 - x1)^2 / R' = the wanted PP (mod p), both in the Montgomery form, or None"""
    s = o.fp_sqrt(wanted_pp_mod_p * RP % P)
    if s is None or s == 0:
        return None
    return on_curve_with_x((p1[0] * RP + s) % P)


def after_first_addition(p1, p2):
    """exact model: the accumulator holds p1 (ZZ = ZZZ = one), p2 is added -> (PP, new accumulator)"""
    x1, y1 = mont(p1)
    x2, y2 = mont(p2)
    Pd = fb.sub28(fb.mm28(x2, ONE), K32, x1)
    PP = fb.mm28(Pd, Pd)
    new, ok = lean_madd28((x1, y1, ONE, ONE), (x2, y2), False)
    return PP, new, ok


def solve_special_points(rng):
    p1 = o.G1.mul(o.G1.gen, rng.randrange(1, o.R))
    found = {}
    # PP with limb 0 zero: PP = k 2^28 in [0.5p, p) -- inside the window [P^2 / R', P^2 / R' + p) of the output for P = 32p .. 34p
    # PP with limb 0 p_0: PP = p + k 2^28, k 2^28 < 0.4p -- the same window holds p + d and not d
    # ZZ' with limb 0 zero: ZZ' = one * PP / R' = PP mod p in [tiny, p + tiny): ZZ' = k 2^28
    while len(found) < 3:
        d = rng.randrange(1, P >> W) << W
        for name, lo, hi in (("pp_zero", P // 2, P), ("pp_p0", 1 << 300, 4 * P // 10), ("zz_zero", 1 << 300, P)):
            if name in found or not lo <= d < hi:
                continue
            p2 = second_point_for(p1, d)
            if p2 is None:
                continue
            PP, new, ok = after_first_addition(p1, p2)
            if not ok:
                continue
            if name == "pp_zero" and PP[0] == 0 or name == "pp_p0" and PP[0] == fb.PL[0] and PP != fb.PL or name == "zz_zero" and new[2][0] == 0:
                found[name] = p2
                break                                                          # one case per point: the three lanes differ
    return p1, found


def test_stream_on_the_inputs_that_pass_the_limb0_tests():
    rng = random.Random(31)
    p1, sp = solve_special_points(rng)
    # the cases are what they claim to be (exact model of the routine's own arithmetic)
    PP, new, _ = after_first_addition(p1, sp["pp_zero"]); assert PP[0] == 0 and any(PP) and PP != fb.PL
    PP, new, _ = after_first_addition(p1, sp["pp_p0"]); assert PP[0] == fb.PL[0] and PP != fb.PL and any(PP[1:])
    PP, new, _ = after_first_addition(p1, sp["zz_zero"]); assert new[2][0] == 0 and any(new[2])
    # a finite row whose x and y both have limb 0 zero (a point of a curve with another b: see the module's docstring)
    odd = ((rng.randrange(1, P >> W) << W) * RINV % P, (rng.randrange(1, P >> W) << W) * RINV % P)
    row = ta.mont_point(odd)
    assert row[0] == 0 and row[N] == 0 and any(row)
    pts = [o.G1.mul(o.G1.gen, rng.randrange(1, o.R)) for _ in range(8)]
    table = pts + [p1, sp["pp_zero"], sp["pp_p0"], sp["zz_zero"], odd, None]
    I1, IPZ, IPP, IZZ, IODD, IINF = range(8, 14)
    NEG = 1 << 31
    lanes = [[I1, IPZ, 0],                  # 0: PP limb 0 zero, PP not zero: no flag, the sum goes on
             [I1, IPP, 1],                  # 1: PP limb 0 p_0, PP not p
             [I1, IZZ, 2],                  # 2: ZZ limb 0 zero after the first addition, then a further point
             [IODD, 3],                     # 3: the limb-0-zero row as the FIRST point of a part (must be taken, not skipped)
             [4, IODD | NEG, 5],            # 4: ... and in the middle of one, negated
             [2, 2, 3],                     # 5: a real doubling
             [6, 6 | NEG],                  # 6: a real cancellation
             [IINF, 7, IINF, 1],            # 7: rows at infinity before and between points
             [IINF, IINF],                  # 8: nothing but infinity
             [0, 1, 2, 3],                  # 9: ordinary
             [5, 4 | NEG, 3, 2 | NEG],      # 10: (outside EXEC below)
             []]                            # 11: empty range
    entries, ranges = [], []
    for l in lanes:
        ranges.append((len(entries), len(entries) + len(l))); entries += l
    for lane in range(len(lanes), LANES):                                      # the rest of the wave: ordinary lanes of every length
        l = [rng.randrange(8) | (rng.randrange(2) << 31)] if lane % 3 == 0 else [k | (rng.randrange(2) << 31) for k in rng.sample(range(8), lane % 4)]
        ranges.append((len(entries), len(entries) + len(l))); entries += l
    exec_mask = ((1 << LANES) - 1) & ~(1 << 10) & ~(1 << 33)
    m, before = run(table, ranges, entries + [0] * 4, exec_mask)
    # both cold blocks ran: the infinity one at least for the first iteration (every accumulator at infinity), the rows at infinity and
    # lane 2's ZZ; the equal-x one for lanes 0, 1 (limb 0 only) and 5, 6 (really equal x)
    assert m.labels.taken.get(".Lvsp_acc28_cold_inf", 0) >= 2 and m.labels.taken.get(".Lvsp_acc28_cold_eqx", 0) >= 1
    assert m.labels.taken.get(".Lvsp_acc28_inf_done", 0) == m.labels.taken[".Lvsp_acc28_cold_inf"]
    assert m.labels.taken.get(".Lvsp_acc28_eqx_done", 0) == m.labels.taken[".Lvsp_acc28_cold_eqx"]
    flags = {5: 1, 6: 1}
    for lane in range(LANES):
        if not (exec_mask >> lane) & 1:
            assert np.array_equal(m.v[:, lane], before[:, lane]), "a lane outside EXEC was touched"
            continue
        a, b = ranges[lane]
        want = ta.expected_sum(table, entries, a, b)
        assert int(m.v[161, lane]) == flags.get(lane, 0), lane
        assert (want == "equal-x") == (lane in flags)
        if lane in flags:
            continue
        if want is None:
            assert not any(ta.lane_result(m, lane)[2]), lane
            continue
        check_lane(m, lane, want)
    assert ta.expected_sum(table, entries, *ranges[3]) == o.G1.add(odd, pts[3])          # the odd row counted as a point


def test_common_path_never_enters_a_cold_block_after_the_first_iteration():
    """ordinary lanes: the cold infinity block runs for the first iteration (all accumulators at infinity) and never again, the equal-x one never"""
    rng = random.Random(32)
    pts = [o.G1.mul(o.G1.gen, rng.randrange(1, o.R)) for _ in range(12)]
    entries, ranges = [], []
    for lane in range(LANES):
        l = [k | (rng.randrange(2) << 31) for k in rng.sample(range(12), 3)]
        ranges.append((len(entries), len(entries) + 3)); entries += l
    m, _ = run(pts, ranges, entries + [0] * 4)
    assert m.labels.taken.get(".Lvsp_acc28_cold_inf", 0) == 1 and ".Lvsp_acc28_cold_eqx" not in m.labels.taken
    assert m.labels.taken[".Lvsp_acc28_loop"] == 2
    for lane in range(LANES):
        assert int(m.v[161, lane]) == 0
        check_lane(m, lane, ta.expected_sum(pts, entries, *ranges[lane]))


# ------------------------------------------------------------------------------------------------ (c) the instruction count
def test_instruction_count_of_one_iteration():
    ins = gen.gen_body()
    a = ins.index(".Lvsp_acc28_loop:")
    backs = [i for i, x in enumerate(ins) if x == "s_cbranch_scc1 .Lvsp_acc28_loop"]
    assert len(backs) == 1
    b = backs[0]
    init = ins.index(".Lvsp_acc28_noinit:")
    first_point = max(i for i, x in enumerate(ins[:init]) if x == "s_cbranch_scc0 .Lvsp_acc28_noinit")
    assert a < first_point < init < b
    # the cold blocks lie behind the back branch and are left through labels of their own
    for lab in (".Lvsp_acc28_cold_inf:", ".Lvsp_acc28_cold_eqx:"):
        assert ins.index(lab) > b
    for lab in (".Lvsp_acc28_inf_done:", ".Lvsp_acc28_eqx_done:"):
        assert a < ins.index(lab) < b
    body = [x for i, x in enumerate(ins[a:b + 1], a) if not x.endswith(":") and not first_point < i < init]
    mad = sum(x.startswith("v_mad_u64_u32") for x in body)
    other = sum(x.startswith("v_") and not x.startswith("v_mad_u64_u32") for x in body)
    assert mad == PARENT_MAD == 3544
    assert other <= PARENT_VALU_OTHER - REMOVED, other
    assert not any(x.startswith("v_mov_b32 v154, 0") or x.startswith("v_mov_b32 v155, 0") for x in ins)
    assert gen.NVGPR <= 168
