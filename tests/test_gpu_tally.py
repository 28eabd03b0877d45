"""GPU: the receiving side of the vote -- batch decompression of G1 points (vsp_g1_decompress_batch) and the tally's aggregation
(vsp_tally_*: common.hpp:1193-1216): decode, check and add ciphertext blobs.  Points are multiples of the generator made by the C
oracle, blobs are written by the oracle's codec, and the expected sums come from the oracle's add_ciphertexts (small sets) and from
the identity  sum_b k_(b,j) G = (sum_b k_(b,j) mod r) G  (every set): the two are checked against each other here."""
import ctypes as C

import numpy as np
import pytest

import bls12_381 as o
import saver
import wire
from conftest import fr_ints_fast, g1_limbs, rand_fr_array

import vote_saver_protocol_amd as v

pytestmark = pytest.mark.gpu

FULL = 27                   # msg_size + 2 of the reference (msg_size = 25)
POOL = 1025                 # ballots in the shared pool: one more than a block of the sum kernel covers (64 lanes x 16 ballots)
# ballot counts: 1, 2, around the 64 lanes of a block, a few blocks' worth of lanes, 1000, around the 1024 ballots of one block
COUNTS = [1, 2, 63, 64, 65, 257, 1000, 1023, 1024, 1025]


class Pool:
    """POOL ballots of FULL points each, made once: scalars, points, compressed bytes.  Ballot b of a tally with ct_len components
    takes the first ct_len points of row b."""

    def __init__(self, cref):
        ks = rand_fr_array(POOL * FULL, 20261)
        self.k = np.array(fr_ints_fast(ks), dtype=object).reshape(POOL, FULL)
        limbs = cref.g1_batch_mul_gen(ks)
        self.pt = [[o.g1_from_limbs([int(t) for t in limbs[b * FULL + j]]) for j in range(FULL)] for b in range(POOL)]
        self.enc = [[o.g1_compress(p) for p in row] for row in self.pt]

    def blob(self, b, ct_len):
        return wire.be(ct_len, 8) + b"".join(self.enc[b][:ct_len])

    def expected(self, ballots, ct_len):
        """[ct_len,12] sums over the ballots (indices into the pool) by the scalar identity"""
        out = np.zeros((ct_len, 12), np.uint64)
        for j in range(ct_len):
            k = sum(int(self.k[b][j]) for b in ballots) % o.R
            out[j] = g1_limbs(o.G1.mul(o.G1.gen, k) if k else None)
        return out


@pytest.fixture(scope="module")
def pool(cref):
    return Pool(cref)


def limbs_of(points):
    return np.array([o.g1_to_limbs(p) for p in points], dtype=np.uint64).reshape(-1, 12)


def oracle_sum(cts):
    return limbs_of(saver.add_ciphertexts(cts))


def host_verdict(enc, check_subgroup):
    try:
        v.g1_decompress(enc, check_subgroup=check_subgroup)
        return True
    except ValueError:
        return False


def tally_of(ctx, ct_len, blobs, check_subgroup=True):
    t = v.Tally(ctx, ct_len)
    try:
        status, accepted = t.add_blobs(blobs, check_subgroup=check_subgroup)
        ct, ballots = t.result()
    finally:
        t.free()
    return status, accepted, ct, ballots


# ---------------------------------------------------------------------------------------------- 1. batch decompression
@pytest.fixture(scope="module")
def three_hundred(pool):
    """300 encodings with the generator, its negation and infinity among them, and what the host function and the oracle make of each"""
    pts = [o.G1.gen, o.G1.neg(o.G1.gen), None] + [p for row in pool.pt[:11] for p in row]
    pts = pts[:300]
    assert len(pts) == 300
    encs = [o.g1_compress(p) for p in pts]
    assert {e[0] & 0x20 for e in encs if e[0] != 0xC0} == {0, 0x20}            # both sign flags occur
    host = np.array([v.g1_decompress(e) for e in encs], dtype=np.uint64)
    assert np.array_equal(host, limbs_of([o.g1_decompress(e) for e in encs])) and np.array_equal(host, limbs_of(pts))
    return encs, host


@pytest.mark.parametrize("n", [1, 64, 65, 300])
def test_batch_decompression_equals_the_host_function_point_by_point(ctx, three_hundred, n):
    encs, host = three_hundred
    for check in (True, False):
        out, status = v.g1_decompress_batch(ctx, b"".join(encs[:n]), check_subgroup=check)
        assert status.shape == (n,) and not status.any()
        assert np.array_equal(out, host[:n])
    # a window that does not start at the generator: the last n of the 300
    out, status = v.g1_decompress_batch(ctx, b"".join(encs[300 - n:]))
    assert not status.any() and np.array_equal(out, host[300 - n:])


# ---------------------------------------------------------------------------------------------- 2. rejections
def bad_encodings():
    """name -> (48 bytes, status with the subgroup check, status without)"""
    good = o.g1_compress(o.G1.mul(o.G1.gen, 5))
    no_flag = bytearray(good); no_flag[0] &= 0x7F
    inf_payload = bytearray(o.g1_compress(None)); inf_payload[47] = 1
    inf_sign = bytearray(o.g1_compress(None)); inf_sign[0] = 0xE0
    x_is_p = bytearray(o.P.to_bytes(48, "big")); x_is_p[0] |= 0x80
    x_is_p_signed = bytearray(x_is_p); x_is_p_signed[0] |= 0x20
    xn = next(x for x in range(5, 200) if o.fp_sqrt((x ** 3 + 4) % o.P) is None)
    non_residue = bytearray(xn.to_bytes(48, "big")); non_residue[0] |= 0x80
    four = bytearray((4).to_bytes(48, "big")); four[0] |= 0x80
    y4 = o.fp_sqrt(68)
    assert y4 is not None and o.G1.is_on_curve((4, y4)) and not o.G1.in_subgroup((4, y4))
    return {"no_compressed_flag": (bytes(no_flag), 1, 1), "infinity_with_payload": (bytes(inf_payload), 1, 1), "infinity_with_sign": (bytes(inf_sign), 1, 1),
            "x_equals_p": (bytes(x_is_p), 1, 1), "x_equals_p_signed": (bytes(x_is_p_signed), 1, 1), "not_on_curve": (bytes(non_residue), 2, 2),
            "outside_subgroup": (bytes(four), 4, 0)}


@pytest.mark.parametrize("check", [True, False])
def test_each_rejection_in_one_lane_among_good_ones(ctx, pool, check):
    good = [e for row in pool.enc[20:24] for e in row][:100]
    bad = bad_encodings()
    encs, want = list(good), [0] * len(good)
    for at, (name, (enc, st_check, st_plain)) in zip((0, 17, 63, 64, 65, 90, 99), bad.items()):
        encs[at] = enc
        want[at] = st_check if check else st_plain
        assert host_verdict(enc, check) == (want[at] == 0), name             # the host function's verdict on the same 48 bytes
    out, status = v.g1_decompress_batch(ctx, b"".join(encs), check_subgroup=check)
    assert status.tolist() == want
    for i, enc in enumerate(encs):
        if want[i]:
            assert not out[i].any()
        else:
            assert np.array_equal(out[i], g1_limbs(o.g1_decompress(enc)))     # with check = 0 this includes the point with x = 4


# ---------------------------------------------------------------------------------------------- 3. tally against the oracle
def test_the_two_expected_sums_agree(pool):
    for ct_len, count in ((3, 65), (FULL, 20)):
        cts = [pool.pt[b][:ct_len] for b in range(count)]
        assert np.array_equal(oracle_sum(cts), pool.expected(range(count), ct_len))


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("ct_len", [3, FULL])
def test_tally_equals_the_oracle(ctx, pool, ct_len, count):
    blobs = [pool.blob(b, ct_len) for b in range(count)]
    assert blobs[0] == wire.g1_vector(pool.pt[0][:ct_len])
    status, accepted, ct, ballots = tally_of(ctx, ct_len, blobs)
    assert status.shape == (count,) and not status.any() and accepted == count and ballots == count
    assert np.array_equal(ct, pool.expected(range(count), ct_len))
    if count <= 65:
        assert np.array_equal(ct, oracle_sum([pool.pt[b][:ct_len] for b in range(count)]))


# ---------------------------------------------------------------------------------------------- 4. chunking
def test_result_does_not_depend_on_how_the_ballots_are_split_over_calls(ctx, pool):
    blobs = [pool.blob(b, FULL) for b in range(1000)]
    _, _, one_call, _ = tally_of(ctx, FULL, b"".join(blobs))
    t = v.Tally(ctx, FULL)
    at = 0
    for part in (1, 63, 64, 65, 807):
        status, accepted = t.add_blobs(blobs[at:at + part])
        at += part
        assert accepted == part and not status.any()
        ct, ballots = t.result()                                               # read in between: adding continues afterwards
        assert ballots == at and np.array_equal(ct, pool.expected(range(at), FULL))
    t.free()
    assert at == 1000 and np.array_equal(ct, one_call)


def test_internal_pieces_give_the_same_result(ctx, pool):
    """a call with many ballots runs in pieces that bound the workspace: with pieces of 100 points (33 ballots of 3, 3 ballots of 27)
    the sums, the statuses and the count are those of one piece"""
    try:
        for ct_len in (3, FULL):
            blobs = [pool.blob(b, ct_len) for b in range(200)]
            bad = bytearray(blobs[150]); bad[8] &= 0x7F; blobs[150] = bytes(bad)
            ctx.set_option("tally_chunk_points", 1 << 21)
            want = tally_of(ctx, ct_len, blobs)
            ctx.set_option("tally_chunk_points", 100)
            got = tally_of(ctx, ct_len, blobs)
            assert got[0].tolist() == want[0].tolist() and got[1] == want[1] == 199 and got[3] == 199
            assert np.array_equal(got[2], want[2]) and np.array_equal(got[2], pool.expected([b for b in range(200) if b != 150], ct_len))
        encs = [e for row in pool.enc[:10] for e in row]
        pts, status = v.g1_decompress_batch(ctx, b"".join(encs))
        assert not status.any() and np.array_equal(pts, limbs_of([p for row in pool.pt[:10] for p in row]))
    finally:
        ctx.set_option("tally_chunk_points", 1 << 21)


# ---------------------------------------------------------------------------------------------- 5. exceptional additions
def exceptional_sets(pool):
    """name -> list of ciphertexts (3 points each)"""
    A, B, Cc = pool.pt[1000][:3], pool.pt[1001][:3], pool.pt[1002][:3]
    return {
        "same_ballot_five_times": [A] * 5,
        "ballot_and_its_negation": [A, [o.G1.neg(p) for p in A]],
        "infinity_components": [[None, A[1], None], [B[0], None, None], [None, None, None], [Cc[0], Cc[1], None]],
        "equal_in_one_component": [A, [B[0], A[1], B[2]]],
    }


@pytest.mark.parametrize("embedded", [False, True])
@pytest.mark.parametrize("name", ["same_ballot_five_times", "ballot_and_its_negation", "infinity_components", "equal_in_one_component"])
def test_exceptional_additions(ctx, pool, name, embedded):
    special = exceptional_sets(pool)[name]
    ordinary = [pool.pt[b][:3] for b in range(100)] if embedded else []
    # the special ballots next to each other in the middle (one lane each, combined in LDS) and, for the doubling, also spread so
    # that one lane meets the same point again (lane stride 64)
    cts = ordinary[:50] + special + ordinary[50:]
    want = oracle_sum(cts)
    if name == "ballot_and_its_negation" and not embedded:
        assert not want.any()                                                  # all infinity
    status, accepted, ct, ballots = tally_of(ctx, 3, [wire.g1_vector(c) for c in cts])
    assert not status.any() and accepted == ballots == len(cts)
    assert np.array_equal(ct, want)
    if embedded:
        spread = list(ordinary)
        for i, c in enumerate(special):
            spread.insert(3 + 64 * i if 3 + 64 * i < len(spread) else len(spread), c)      # ballots 3, 67, ...: the same lane of the block
        status, accepted, ct, _ = tally_of(ctx, 3, [wire.g1_vector(c) for c in spread])
        assert accepted == len(spread) and np.array_equal(ct, oracle_sum(spread))


def test_running_sum_passes_through_infinity(ctx, pool):
    A, B = pool.pt[1003][:3], pool.pt[1004][:3]
    neg = lambda ct: [o.G1.neg(p) for p in ct]
    t = v.Tally(ctx, 3)
    t.add_blobs([wire.g1_vector(A)])
    t.add_blobs([wire.g1_vector(neg(A))])
    ct, ballots = t.result()
    assert not ct.any() and ballots == 2
    t.add_blobs([wire.g1_vector(B), wire.g1_vector(B)])                        # and a doubling inside one call, folded into an infinite sum
    ct, ballots = t.result()
    assert ballots == 4 and np.array_equal(ct, limbs_of([o.G1.add(p, p) for p in B]))
    t.add_blobs([wire.g1_vector(neg(B))])                                      # host fold: 2B + (-B)
    assert np.array_equal(t.result()[0], limbs_of(B))
    t.free()


# ---------------------------------------------------------------------------------------------- 6. rejected ballots
def test_rejected_ballots_contribute_nothing(ctx, pool):
    ct_len = 3
    blobs = [pool.blob(b, ct_len) for b in range(100)]
    bad = bad_encodings()

    def corrupt(b, j, enc):
        x = bytearray(blobs[b]); x[8 + 48 * j:56 + 48 * j] = enc; blobs[b] = bytes(x)

    corrupt(5, 0, bad["no_compressed_flag"][0])             # bit 0
    corrupt(40, 2, bad["not_on_curve"][0])                  # bit 1
    corrupt(64, 1, bad["outside_subgroup"][0])              # bit 2
    corrupt(77, 0, bad["x_equals_p"][0]); corrupt(77, 1, bad["not_on_curve"][0]); corrupt(77, 2, bad["outside_subgroup"][0])      # all three
    hdr = bytearray(blobs[99]); hdr[:8] = wire.be(ct_len + 1, 8); blobs[99] = bytes(hdr)        # count header
    want = np.zeros(100, np.uint8)
    want[5], want[40], want[64], want[77], want[99] = 1, 2, 4, 7, 1
    good = [b for b in range(100) if not want[b]]
    t = v.Tally(ctx, ct_len)
    status, accepted = t.add_blobs(b"".join(blobs))
    ct, ballots = t.result()
    assert status.tolist() == want.tolist() and accepted == ballots == 95
    assert np.array_equal(ct, pool.expected(good, ct_len)) and np.array_equal(ct, oracle_sum([pool.pt[b][:ct_len] for b in good]))
    # without the subgroup check ballot 64 is accepted and the sum is the exact curve sum
    t.reset()
    assert not t.result()[0].any() and t.result()[1] == 0
    status, accepted = t.add_blobs(blobs, check_subgroup=False)
    want[64], want[77] = 0, 3
    assert status.tolist() == want.tolist() and accepted == 96
    ct64 = list(pool.pt[64][:ct_len]); ct64[1] = o.g1_decompress(bad["outside_subgroup"][0])
    assert np.array_equal(t.result()[0], oracle_sum([pool.pt[b][:ct_len] for b in good] + [ct64]))
    # every ballot rejected: infinity and 0; then a reset and a fresh, correct tally
    t.reset()
    status, accepted = t.add_blobs([blobs[5], blobs[40], blobs[99]])
    ct, ballots = t.result()
    assert status.tolist() == [1, 2, 1] and accepted == 0 and ballots == 0 and not ct.any()
    t.reset()
    ct, ballots = t.result()
    assert not ct.any() and ballots == 0
    status, accepted = t.add_blobs([pool.blob(b, ct_len) for b in range(10)])
    ct, ballots = t.result()
    assert accepted == ballots == 10 and np.array_equal(ct, pool.expected(range(10), ct_len))
    t.free()


# ---------------------------------------------------------------------------------------------- 7. argument errors
def test_argument_errors_leave_the_context_usable(ctx, pool):
    lib, h = ctx.lib, ctx.h
    ERR_ARG = -1
    blob = np.frombuffer(pool.blob(0, 3), dtype=np.uint8)
    status = np.zeros(4, np.uint8); acc = C.c_size_t(0); out = np.zeros((3, 12), np.uint64); n = C.c_uint64(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert not lib.vsp_tally_create(h, 0) and "ct_len" in ctx.last_error()
    assert not lib.vsp_tally_create(h, 1025)
    assert not lib.vsp_tally_create(None, 3)
    t = lib.vsp_tally_create(h, 1024)
    assert t
    lib.vsp_tally_free(h, t)
    t = lib.vsp_tally_create(h, 3)
    assert lib.vsp_tally_add_blobs(h, None, p(blob), 1, 1, p(status), C.byref(acc)) == ERR_ARG
    assert lib.vsp_tally_add_blobs(h, t, None, 1, 1, p(status), C.byref(acc)) == ERR_ARG
    assert lib.vsp_tally_add_blobs(h, t, None, 0, 1, None, None) == ERR_ARG
    assert lib.vsp_tally_add_blobs(None, t, p(blob), 1, 1, None, None) == ERR_ARG
    assert lib.vsp_tally_result(h, None, p(out), C.byref(n)) == ERR_ARG
    assert lib.vsp_tally_result(h, t, None, C.byref(n)) == ERR_ARG
    assert lib.vsp_tally_reset(h, None) == ERR_ARG
    enc = np.frombuffer(pool.enc[0][0], dtype=np.uint8)
    assert lib.vsp_g1_decompress_batch(h, None, 1, 1, p(out), p(status)) == ERR_ARG
    assert lib.vsp_g1_decompress_batch(h, p(enc), 1, 1, None, p(status)) == ERR_ARG
    assert lib.vsp_g1_decompress_batch(h, p(enc), 1, 1, p(out), None) == ERR_ARG
    assert lib.vsp_g1_decompress_batch(None, p(enc), 1, 1, p(out), p(status)) == ERR_ARG
    # nothing above touched the handle; the context and the handle still work: optional outputs left out, an empty call, a result
    assert lib.vsp_tally_add_blobs(h, t, p(blob), 0, 1, None, None) == 0
    assert lib.vsp_tally_add_blobs(h, t, p(blob), 1, 1, None, None) == 0
    assert lib.vsp_tally_result(h, t, p(out), None) == 0
    assert np.array_equal(out, limbs_of(pool.pt[0][:3]))
    assert lib.vsp_g1_decompress_batch(h, p(enc), 0, 1, p(out), p(status)) == 0
    lib.vsp_tally_free(h, t)
    lib.vsp_tally_free(h, None)
    with pytest.raises(v.VspError):
        v.Tally(ctx, 0)
    with pytest.raises(ValueError):
        v.g1_decompress_batch(ctx, b"\x00" * 47)
    pts, st = v.g1_decompress_batch(ctx, pool.enc[0][0])
    assert not st.any() and np.array_equal(pts, limbs_of([pool.pt[0][0]]))
