"""GPU: decoding proofs on the receiving side -- batch decompression of G2 points (vsp_g2_decompress_batch) and of whole proof blobs
(vsp_proof_from_blob_batch: A | B | C, the layout of data.bin[0:192)).  Points are multiples of the generators made by the C oracle,
encoded by the oracle's codec; the yardsticks are the library's host functions (vsp_g2_decompress, vsp_proof_from_blob) and the
oracle's decoder."""
import ctypes as C
import os

import numpy as np
import pytest

import bls12_381 as o
from conftest import GOLDEN, g1_limbs, g2_limbs, rand_fr_array

import vote_saver_protocol_amd as v

pytestmark = pytest.mark.gpu

NPTS = 300                  # G2 points in the shared pool
NPROOFS = 257               # proofs in the shared pool: one more than a block of the decoding kernels covers
ERR_ARG = -1
CHUNK_DEFAULT = 1 << 21


class Pool:
    """made once: 297 multiples of the G2 generator (+ the generator, its negation, infinity = 300 encodings) with what the host function
    makes of each, and 2 x 257 multiples of the G1 generator: proof k is A = g1[k], B = g2[k], C = g1[257 + k]"""

    def __init__(self, cref):
        l2 = cref.g2_batch_mul_gen(rand_fr_array(NPTS - 3, 20270))
        self.pt2 = [o.G2.gen, o.G2.neg(o.G2.gen), None] + [o.g2_from_limbs([int(t) for t in row]) for row in l2]
        self.enc2 = [o.g2_compress(p) for p in self.pt2]
        self.host2 = np.array([v.g2_decompress(e) for e in self.enc2], dtype=np.uint64)
        l1 = cref.g1_batch_mul_gen(rand_fr_array(2 * NPROOFS, 20271))
        self.pt1 = [o.g1_from_limbs([int(t) for t in row]) for row in l1]
        self.pt1[2] = None                                                      # proof 2: A is infinity
        self.pt1[NPROOFS + 6] = None                                            # proof 6: C is infinity
        self.enc1 = [o.g1_compress(p) for p in self.pt1]
        # proof k's B is G2 pool point k + 1, so that proof 1's B is infinity and proof 0's the generator's negation
        self.blobs = [self.enc1[k] + self.enc2[k + 1] + self.enc1[NPROOFS + k] for k in range(NPROOFS)]
        self.host_proofs = [v.proof_from_blob(b) for b in self.blobs]           # with the subgroup check: every member is in the subgroup


@pytest.fixture(scope="module")
def pool(cref):
    return Pool(cref)


def host_verdict(fn, enc, check_subgroup):
    try:
        fn(enc, check_subgroup=check_subgroup)
        return True
    except ValueError:
        return False


# ---------------------------------------------------------------------------------------------- 1. point by point
def test_the_yardsticks_agree(pool):
    assert {e[0] & 0x20 for e in pool.enc2 if e[0] != 0xC0} == {0, 0x20}       # both sign flags occur
    oracle = np.array([g2_limbs(o.g2_decompress(e)) for e in pool.enc2], dtype=np.uint64)
    assert np.array_equal(pool.host2, oracle)
    assert np.array_equal(pool.host2, np.array([g2_limbs(p) for p in pool.pt2], dtype=np.uint64))
    assert not pool.host2[2].any()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 300])
def test_batch_decompression_equals_the_host_function_point_by_point(ctx, pool, n):
    for check in (True, False):
        out, status = v.g2_decompress_batch(ctx, b"".join(pool.enc2[:n]), check_subgroup=check)
        assert out.shape == (n, 24) and status.shape == (n,) and not status.any()
        assert np.array_equal(out, pool.host2[:n])
    # a window that does not start at the generator: the last n of the 300
    out, status = v.g2_decompress_batch(ctx, b"".join(pool.enc2[NPTS - n:]))
    assert not status.any() and np.array_equal(out, pool.host2[NPTS - n:])


def test_internal_pieces_give_the_same_result(ctx, pool):
    """pieces of 100 points: 300 G2 points cross two boundaries, 257 proofs (33 per piece) cross seven"""
    try:
        ctx.set_option("tally_chunk_points", 100)
        out, status = v.g2_decompress_batch(ctx, b"".join(pool.enc2))
        assert not status.any() and np.array_equal(out, pool.host2)
        bad = list(pool.enc2); bad[199] = bad_g2()["not_on_curve"][0]
        out, status = v.g2_decompress_batch(ctx, b"".join(bad))
        assert status.tolist() == [0] * 199 + [2] + [0] * 100 and not out[199].any() and np.array_equal(out[200:], pool.host2[200:])
        blobs = list(pool.blobs); blobs[133] = blobs[133][:48] + bad_g2()["c1_equals_p"][0] + blobs[133][144:]
        check_proofs(ctx, pool, blobs, {133: 0x21}, True)
    finally:
        ctx.set_option("tally_chunk_points", CHUNK_DEFAULT)


def test_stage_times_are_reported(ctx, pool):
    stages = ("g2_decode_ms", "g2_subgroup_ms")
    ctx.stats_reset()
    assert [ctx.stat(s) for s in stages] == [0, 0]
    v.g2_decompress_batch(ctx, b"".join(pool.enc2[:64]), check_subgroup=False)
    assert ctx.stat("g2_decode_ms") > 0 and ctx.stat("g2_subgroup_ms") == 0
    first = ctx.stat("g2_decode_ms")
    v.proofs_from_blob_batch(ctx, b"".join(pool.blobs[:64]))
    assert ctx.stat("g2_decode_ms") > first and ctx.stat("g2_subgroup_ms") > 0          # summed since the reset


def test_proof_path_counts_each_group_into_its_own_stage_stats(ctx, pool):
    """A and C of a proof count into the G1 stages, B into the G2 stages, nothing into the tally's sum; a G1 call afterwards moves
    the G1 decoding time alone"""
    stages = ("tally_decode_ms", "tally_subgroup_ms", "g2_decode_ms", "g2_subgroup_ms")
    ctx.stats_reset()
    v.proofs_from_blob_batch(ctx, b"".join(pool.blobs[:65]), check_subgroup=True)
    after_proofs = [ctx.stat(s) for s in stages]
    assert all(t > 0 for t in after_proofs) and ctx.stat("tally_sum_ms") == 0
    v.g1_decompress_batch(ctx, b"".join(pool.enc1[:65]), check_subgroup=False)
    assert ctx.stat("tally_decode_ms") > after_proofs[0]
    assert [ctx.stat(s) for s in stages[1:]] == after_proofs[1:] and ctx.stat("tally_sum_ms") == 0


# ---------------------------------------------------------------------------------------------- 2. rejections
def flagged(value_bytes):
    b = bytearray(value_bytes); b[0] |= 0x80
    return bytes(b)


def bad_g2():
    """name -> (96 bytes, status with the subgroup check, status without)"""
    good = o.g2_compress(o.G2.mul(o.G2.gen, 5))
    be = lambda x: x.to_bytes(48, "big")
    no_flag = bytearray(good); no_flag[0] &= 0x7F
    inf_payload = bytearray(o.g2_compress(None)); inf_payload[95] = 1
    inf_sign = bytearray(o.g2_compress(None)); inf_sign[0] = 0xE0
    x2 = (2, 0)
    y2 = o.fp2_sqrt(o.Fp2Ops.add(o.Fp2Ops.mul(o.Fp2Ops.sqr(x2), x2), (4, 4)))
    assert y2 is not None and o.G2.is_on_curve((x2, y2)) and not o.G2.in_subgroup((x2, y2))
    assert o.fp2_sqrt((5, 4)) is None                                           # x = (1, 0): 1 + 4 (1 + u) is no square
    return {"no_compressed_flag": (bytes(no_flag), 1, 1), "infinity_with_payload": (bytes(inf_payload), 1, 1), "infinity_with_sign": (bytes(inf_sign), 1, 1),
            "c1_equals_p": (flagged(be(o.P) + be(3)), 1, 1), "c0_equals_p": (flagged(be(1) + be(o.P)), 1, 1),
            "not_on_curve": (flagged(be(0) + be(1)), 2, 2), "outside_subgroup": (flagged(be(0) + be(2)), 4, 0)}


def bad_g1():
    """the same kinds for a 48-byte member of a proof"""
    good = o.g1_compress(o.G1.mul(o.G1.gen, 5))
    no_flag = bytearray(good); no_flag[0] &= 0x7F
    inf_payload = bytearray(o.g1_compress(None)); inf_payload[47] = 1
    inf_sign = bytearray(o.g1_compress(None)); inf_sign[0] = 0xE0
    xn = next(x for x in range(5, 200) if o.fp_sqrt((x ** 3 + 4) % o.P) is None)
    y4 = o.fp_sqrt(68)
    assert y4 is not None and not o.G1.in_subgroup((4, y4))
    return {"no_compressed_flag": (bytes(no_flag), 1, 1), "infinity_with_payload": (bytes(inf_payload), 1, 1), "infinity_with_sign": (bytes(inf_sign), 1, 1),
            "x_equals_p": (flagged(o.P.to_bytes(48, "big")), 1, 1), "not_on_curve": (flagged(xn.to_bytes(48, "big")), 2, 2),
            "outside_subgroup": (flagged((4).to_bytes(48, "big")), 4, 0)}


@pytest.mark.parametrize("positions", [(0, 1, 62, 63, 64, 65, 66), (65, 64, 63, 0, 99, 66, 1)])
@pytest.mark.parametrize("check", [True, False])
def test_each_rejection_in_one_lane_among_good_ones(ctx, pool, check, positions):
    encs, want = list(pool.enc2[100:200]), [0] * 100
    for at, (name, (enc, st_check, st_plain)) in zip(positions, bad_g2().items()):
        encs[at] = enc
        want[at] = st_check if check else st_plain
        assert host_verdict(v.g2_decompress, enc, check) == (want[at] == 0), name          # the host function's verdict on the same 96 bytes
    out, status = v.g2_decompress_batch(ctx, b"".join(encs), check_subgroup=check)
    assert status.tolist() == want
    for i, enc in enumerate(encs):
        if want[i]:
            assert not out[i].any()
        elif i in positions:
            assert np.array_equal(out[i], g2_limbs(o.g2_decompress(enc)))                  # check = 0: the point with x = (2, 0)
            assert np.array_equal(out[i], v.g2_decompress(enc, check_subgroup=False))
        else:
            assert np.array_equal(out[i], pool.host2[100 + i])


# ---------------------------------------------------------------------------------------------- 3. proofs
def test_the_reference_proof_decodes_and_reencodes(ctx):
    d = bytes.fromhex(open(os.path.join(GOLDEN, "data_bin_proof.hex")).read().strip())
    assert len(d) == 192
    A, B, Cc, status = v.proofs_from_blob_batch(ctx, d)
    hA, hB, hC = v.proof_from_blob(d)
    assert status.tolist() == [0]
    assert np.array_equal(A[0], hA) and np.array_equal(B[0], hB) and np.array_equal(Cc[0], hC)
    assert v.g1_compress(A[0]) + v.g2_compress(B[0]) + v.g1_compress(Cc[0]) == d


MEMBER = {"A": (0, 48, 0x10), "B": (48, 144, 0x20), "C": (144, 192, 0x40)}
# (proof, member, kind): every kind of damage in every member it applies to, at the block's edges too, and one proof with all three damaged
DAMAGE = [(3, "A", "no_compressed_flag"), (5, "B", "no_compressed_flag"), (7, "C", "infinity_with_payload"), (9, "B", "infinity_with_payload"),
          (11, "A", "infinity_with_sign"), (13, "B", "infinity_with_sign"), (20, "B", "c1_equals_p"), (22, "B", "c0_equals_p"), (24, "C", "x_equals_p"),
          (30, "A", "not_on_curve"), (32, "B", "not_on_curve"), (40, "C", "outside_subgroup"), (42, "B", "outside_subgroup"),
          (50, "A", "no_compressed_flag"), (50, "B", "not_on_curve"), (50, "C", "outside_subgroup"),
          (63, "B", "not_on_curve"), (64, "A", "outside_subgroup"), (200, "C", "not_on_curve"), (256, "B", "outside_subgroup")]


def damaged(pool, n, plan, check):
    """(blobs, {proof: expected status}) for the first n proofs of the pool with the plan's entries below n applied"""
    b1, b2 = bad_g1(), bad_g2()
    blobs, want = [bytearray(b) for b in pool.blobs[:n]], {}
    for k, member, kind in plan:
        if k >= n:
            continue
        enc, st_check, st_plain = (b2 if member == "B" else b1)[kind]
        lo, hi, bit = MEMBER[member]
        blobs[k][lo:hi] = enc
        st = st_check if check else st_plain
        if st:
            want[k] = want.get(k, 0) | st | bit
    return [bytes(b) for b in blobs], want


def check_proofs(ctx, pool, blobs, want, check):
    """the batch's statuses are `want` (0 where absent); rejected proofs are all zero; accepted ones equal the host function's output"""
    n = len(blobs)
    A, B, Cc, status = v.proofs_from_blob_batch(ctx, b"".join(blobs), check_subgroup=check)
    assert A.shape == (n, 12) and B.shape == (n, 24) and Cc.shape == (n, 12)
    assert status.tolist() == [want.get(k, 0) for k in range(n)]
    for k in range(n):
        if k in want or blobs[k] != pool.blobs[k]:
            assert host_verdict(v.proof_from_blob, blobs[k], check) == (k not in want), k   # the host function's verdict on the same 192 bytes
        if k in want:
            assert not A[k].any() and not B[k].any() and not Cc[k].any(), k
        else:
            hA, hB, hC = pool.host_proofs[k] if blobs[k] == pool.blobs[k] else v.proof_from_blob(blobs[k], check_subgroup=check)
            assert np.array_equal(A[k], hA) and np.array_equal(B[k], hB) and np.array_equal(Cc[k], hC), k
    return A, B, Cc, status


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_proofs_equal_the_host_function_and_rejections_are_reported(ctx, pool, n):
    assert not pool.host_proofs[2][0].any() and not pool.host_proofs[1][1].any() and not pool.host_proofs[6][2].any()      # infinity members
    for check in (True, False):
        check_proofs(ctx, pool, pool.blobs[:n], {}, check)
        plan = DAMAGE if n > 1 else [(0, "B", "not_on_curve")]
        blobs, want = damaged(pool, n, plan, check)
        assert want and (n < 64 or want[50] == (0x77 if check else 0x33))
        A, B, Cc, status = check_proofs(ctx, pool, blobs, want, check)
        # outputs left out: B alone, then all three
        lib, p = ctx.lib, lambda a: a.ctypes.data_as(C.c_void_p)
        buf = np.frombuffer(b"".join(blobs), dtype=np.uint8)
        A2, C2, st2 = np.ones((n, 12), np.uint64), np.ones((n, 12), np.uint64), np.ones(n, np.uint8)
        assert lib.vsp_proof_from_blob_batch(ctx.h, p(buf), n, int(check), p(A2), None, p(C2), p(st2)) == 0
        assert np.array_equal(A2, A) and np.array_equal(C2, Cc) and np.array_equal(st2, status)
        st3 = np.ones(n, np.uint8)
        assert lib.vsp_proof_from_blob_batch(ctx.h, p(buf), n, int(check), None, None, None, p(st3)) == 0
        assert np.array_equal(st3, status)


# ---------------------------------------------------------------------------------------------- 4. argument errors
def test_argument_errors_leave_the_context_usable(ctx, pool):
    lib, h = ctx.lib, ctx.h
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    enc = np.frombuffer(pool.enc2[3], dtype=np.uint8)
    blob = np.frombuffer(pool.blobs[0], dtype=np.uint8)
    out = np.zeros((1, 24), np.uint64); A = np.zeros((1, 12), np.uint64); Cc = np.zeros((1, 12), np.uint64); status = np.ones(1, np.uint8)
    assert lib.vsp_g2_decompress_batch(h, None, 1, 1, p(out), p(status)) == ERR_ARG and "g2_decompress_batch" in ctx.last_error()
    assert lib.vsp_g2_decompress_batch(h, p(enc), 1, 1, None, p(status)) == ERR_ARG
    assert lib.vsp_g2_decompress_batch(h, p(enc), 1, 1, p(out), None) == ERR_ARG
    assert lib.vsp_g2_decompress_batch(h, None, 0, 1, p(out), p(status)) == ERR_ARG
    assert lib.vsp_g2_decompress_batch(None, p(enc), 1, 1, p(out), p(status)) == ERR_ARG
    assert lib.vsp_proof_from_blob_batch(h, None, 1, 1, p(A), p(out), p(Cc), p(status)) == ERR_ARG and "proof_from_blob_batch" in ctx.last_error()
    assert lib.vsp_proof_from_blob_batch(h, p(blob), 1, 1, p(A), p(out), p(Cc), None) == ERR_ARG
    assert lib.vsp_proof_from_blob_batch(h, None, 0, 1, p(A), p(out), p(Cc), p(status)) == ERR_ARG
    assert lib.vsp_proof_from_blob_batch(None, p(blob), 1, 1, p(A), p(out), p(Cc), p(status)) == ERR_ARG
    assert not out.any() and status[0] == 1                                    # nothing was written
    # the context still works: empty calls, then good ones
    assert lib.vsp_g2_decompress_batch(h, p(enc), 0, 1, p(out), p(status)) == 0
    assert lib.vsp_proof_from_blob_batch(h, p(blob), 0, 1, p(A), p(out), p(Cc), p(status)) == 0
    assert lib.vsp_g2_decompress_batch(h, p(enc), 1, 1, p(out), p(status)) == 0
    assert status[0] == 0 and np.array_equal(out[0], pool.host2[3])
    assert lib.vsp_proof_from_blob_batch(h, p(blob), 1, 1, p(A), p(out), p(Cc), p(status)) == 0
    assert status[0] == 0 and np.array_equal(A[0], pool.host_proofs[0][0]) and np.array_equal(out[0], pool.host_proofs[0][1])
    with pytest.raises(ValueError):
        v.g2_decompress_batch(ctx, b"\x00" * 95)
    with pytest.raises(ValueError):
        v.proofs_from_blob_batch(ctx, b"\x00" * 191)
    pts, st = v.g2_decompress_batch(ctx, pool.enc2[0])
    assert not st.any() and np.array_equal(pts[0], g2_limbs(o.G2.gen))
