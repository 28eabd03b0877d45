"""GPU tests of the Pedersen hash over Jubjub (vsp_pedersen_hash_batch) against the big-integer model tests/jubjub_model.py, bit for bit:
every message length at which the schedule changes, counts around a wave and a workgroup, every lane-group size and the automatic
choice, all-zero and all-one messages, digests with and without points; partial sums that coincide or cancel inside the fold; the
generators that vsp_pedersen_create must refuse; the argument errors."""
import ctypes as C
import random

import numpy as np
import pytest

import jubjub_model as jm
import vote_saver_protocol_amd as v

pytestmark = pytest.mark.gpu

G = 3
SIZES = [1, 2, 3, 4, 188, 189, 190, 255, 378, 510, 189 * G]
COUNTS = [1, 63, 64, 65, 257]
LANES = [0, 1, 4, 16, 64]                                            # option "pedersen_lanes": 0 = automatic
ERR_ARG = -1
MINUS_ONE = (0, jm.R - 1)


def gen_array(gens):
    return np.array([jm.point_words(g) for g in gens], np.uint64)


def msg_array(messages):
    return np.array([jm.message_words(bits) for bits in messages], np.uint64)


@pytest.fixture(scope="module")
def gens():
    return jm.generators(G)


@pytest.fixture(scope="module")
def ped(ctx, gens):
    h = v.Pedersen(ctx, gen_array(gens))
    yield h
    h.free()


@pytest.fixture(scope="module")
def reference(gens):
    """per message length: 257 messages (random, the all-zero one at index 1, the all-one one at index 2) and their hash points, once"""
    model = jm.Table(gens)
    rng = random.Random(21)
    ref = {}
    for n in SIZES:
        messages = [[rng.getrandbits(1) for _ in range(n)] for _ in range(max(COUNTS))]
        messages[1] = [0] * n
        messages[2] = [1] * n
        points = [model.hash_point(bits) for bits in messages]
        ref[n] = (msg_array(messages), np.array([jm.point_words(q) for q in points], np.uint64))
    return ref


@pytest.fixture
def lanes_option(ctx):
    yield lambda value: ctx.set_option("pedersen_lanes", value)
    ctx.set_option("pedersen_lanes", 0)


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("n", SIZES)
def test_hash_batch_against_the_model(ctx, ped, reference, lanes_option, n, lanes):
    msgs, points = reference[n]
    lanes_option(lanes)
    for count in COUNTS:
        digests = v.pedersen_hash_batch(ctx, ped, msgs[:count], n)
        assert np.array_equal(digests, points[:count, :4]), (n, lanes, count)
        d2, pts = v.pedersen_hash_batch(ctx, ped, msgs[:count], n, points=True)
        assert np.array_equal(d2, digests) and np.array_equal(pts, points[:count]), (n, lanes, count)
    assert not (digests[:, 3] >> np.uint64(63)).any()               # 255 bits


def test_handle_reports_its_sizes(ctx, ped):
    assert ped.generators == G and ped.max_bits == 189 * G
    assert ped.device_bytes() >= G * 63 * 4 * 96
    before = ctx.stat("pedersen_ms")
    v.pedersen_hash_batch(ctx, ped, np.zeros((4, 1), np.uint64), 3)
    assert ctx.stat("pedersen_ms") > before


def test_stray_bits_above_n_are_ignored(ctx, ped, reference):
    for n in (1, 4, 190, 255, 510):
        msgs, points = reference[n]
        dirty = msgs[:65].copy()
        dirty[:, -1] |= np.uint64((0xFFFFFFFFFFFFFFFF << (n % 64)) & 0xFFFFFFFFFFFFFFFF)
        assert not np.array_equal(dirty, msgs[:65])
        assert np.array_equal(v.pedersen_hash_batch(ctx, ped, dirty, n), points[:65, :4])


@pytest.mark.parametrize("lanes", LANES)
def test_coinciding_and_cancelling_partial_sums(ctx, gens, lanes_option, lanes):
    """generators G_1 = G_0 (accepted: independence is the caller's business).  A 378-bit message whose second segment repeats the first
    doubles inside the fold; with every s2 of the second segment flipped the sum is the identity: digest 0, point (0, 1)"""
    same = [gens[0], gens[0]]
    with v.Pedersen(ctx, gen_array(same)) as twin:
        model = jm.Table(same)
        rng = random.Random(22)
        firsts = [[rng.getrandbits(1) for _ in range(189)] for _ in range(5)]
        doubled = [f + f for f in firsts]
        cancelled = [f + [b ^ 1 if k % 3 == 2 else b for k, b in enumerate(f)] for f in firsts]
        lanes_option(lanes)
        d, pts = v.pedersen_hash_batch(ctx, twin, msg_array(doubled), 378, points=True)
        want = [model.hash_point(m) for m in doubled]
        assert want[0] == jm.add(model.hash_point(firsts[0]), model.hash_point(firsts[0]))
        assert pts.tolist() == [jm.point_words(q) for q in want] and np.array_equal(d, pts[:, :4])
        d, pts = v.pedersen_hash_batch(ctx, twin, msg_array(cancelled), 378, points=True)
        assert not d.any() and pts.tolist() == [jm.point_words(jm.IDENTITY)] * 5


def test_create_refuses_bad_generators_and_names_them(ctx, gens):
    raw = jm.uncleared_point()
    off = (gens[0][0], (gens[0][1] + 1) % jm.R)
    too_big = jm.words(gens[0][0] + jm.R) + jm.words(gens[0][1])
    for bad, why in ((jm.point_words(off), "not on the curve"), (jm.point_words(jm.IDENTITY), "identity"), (jm.point_words(MINUS_ONE), "prime order"),
                     (jm.point_words(raw), "prime order"), (too_big, "not below r")):
        for at in (0, 2):
            rows = [jm.point_words(g) for g in gens]
            rows[at] = bad
            with pytest.raises(v.VspError) as e:
                v.Pedersen(ctx, np.array(rows, np.uint64))
            assert "vsp error -1" in str(e.value) and f"generator {at} " in str(e.value) and why in str(e.value), str(e.value)
    with v.Pedersen(ctx, gen_array([gens[1], gens[1], jm.neg(gens[1])])) as h:      # equal and opposite generators are accepted
        assert h.generators == 3


def test_argument_errors(ctx, ped):
    lib = ctx.lib
    msgs = np.zeros((2, 9), np.uint64); out = np.zeros((2, 4), np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    ok = lambda: lib.vsp_pedersen_hash_batch(ctx.h, ped.h, p(msgs), 510, 2, p(out), None)
    assert ok() == 0
    assert lib.vsp_pedersen_hash_batch(ctx.h, ped.h, p(msgs), 510, 0, p(out), None) == 0            # count 0 with valid pointers
    assert lib.vsp_pedersen_hash_batch(ctx.h, None, p(msgs), 510, 2, p(out), None) == ERR_ARG
    assert lib.vsp_pedersen_hash_batch(ctx.h, ped.h, None, 510, 0, p(out), None) == ERR_ARG         # a null pointer even with count 0
    assert lib.vsp_pedersen_hash_batch(ctx.h, ped.h, p(msgs), 510, 0, None, None) == ERR_ARG
    assert lib.vsp_pedersen_hash_batch(None, ped.h, p(msgs), 510, 2, p(out), None) == ERR_ARG
    assert lib.vsp_pedersen_hash_batch(ctx.h, ped.h, p(msgs), 0, 2, p(out), None) == ERR_ARG        # n = 0 bits
    assert lib.vsp_pedersen_hash_batch(ctx.h, ped.h, p(msgs), 189 * G + 1, 2, p(out), None) == ERR_ARG
    assert "189 g" in ctx.last_error()
    assert lib.vsp_pedersen_hash_batch(ctx.h, ped.h, p(msgs), 189 * G, 2, p(out), None) == 0
    h = C.c_void_p(None)
    gens = np.zeros((1, 8), np.uint64)
    assert lib.vsp_pedersen_create(ctx.h, None, 1, C.byref(h)) == ERR_ARG and not h.value
    assert lib.vsp_pedersen_create(ctx.h, p(gens), 1, None) == ERR_ARG
    assert lib.vsp_pedersen_create(ctx.h, p(gens), 0, C.byref(h)) == ERR_ARG and not h.value
    assert lib.vsp_pedersen_generators(None) == 0 and lib.vsp_pedersen_max_bits(None) == 0
    assert ok() == 0                                                 # the context is usable after every refusal
