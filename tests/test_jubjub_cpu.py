"""CPU build of the registry's rules: vote_saver_protocol_amd/csrc/jubjub.h compiled by g++ (64-bit limbs) and compared, bit for bit,
with the big-integer model tests/jubjub_model.py -- the group law at its special inputs, the mixed addition with negated entries, the
chunk encoding, the schedule, stray bits, the lane shares and the fold order of every group size, the generator tests, the blob bit
order and the rt split.  Every hash case is computed by both routes of the model (the definition and the windowed one), which must
agree.  No GPU."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import jubjub_model as jm
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpu_build", "jubjub_check.cpp")
G = 3
SIZES = [1, 2, 3, 4, 188, 189, 190, 255, 378, 510, 189 * G]
LANES = [1, 4, 16, 64]
MINUS_ONE = (0, jm.R - 1)                                            # the point of order 2


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def pt(point):
    return np.array(jm.point_words(point), np.uint64)


@pytest.fixture(scope="module")
def jj(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cpu_build") / "libjjchk.so")
    flags = os.environ.get("VSP_MATHCHK_FLAGS", "-O2").split()
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.chk_jj_table_new.restype = C.c_void_p
    lib.chk_jj_table_new.argtypes = [C.c_void_p, C.c_size_t]
    lib.chk_jj_table_free.argtypes = [C.c_void_p]
    lib.chk_jj_table_window.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint]
    lib.chk_jj_hash.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.chk_jj_tree.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_int, C.c_void_p]
    lib.chk_jj_schedule.restype = C.c_size_t
    lib.chk_jj_schedule.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p]
    lib.chk_jj_max_bits.restype = C.c_size_t
    lib.chk_jj_max_bits.argtypes = [C.c_size_t]
    lib.chk_jj_message_bit.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
    lib.chk_jj_level_first.restype = C.c_uint64
    lib.chk_jj_sibling.restype = C.c_uint64
    lib.chk_jj_sibling.argtypes = [C.c_uint64, C.c_uint]
    return lib


@pytest.fixture(scope="module")
def gens():
    return jm.generators(G)


@pytest.fixture(scope="module")
def model(gens):
    return jm.Table(gens)


@pytest.fixture(scope="module")
def table(jj, gens):
    ga = np.array([jm.point_words(g) for g in gens], np.uint64)
    t = jj.chk_jj_table_new(p(ga), G)
    yield C.c_void_p(t), ga
    jj.chk_jj_table_free(C.c_void_p(t))


def lib_add(jj, a, b):
    out = np.zeros(8, np.uint64)
    jj.chk_jj_add(p(pt(a)), p(pt(b)), p(out))
    return out.tolist()


def test_unified_addition_at_its_special_inputs(jj, gens):
    P, Q = gens[0], gens[1]
    cases = [(P, Q), (Q, P), (P, P), (P, jm.neg(P)), (jm.IDENTITY, P), (P, jm.IDENTITY), (jm.IDENTITY, jm.IDENTITY),
             (MINUS_ONE, P), (P, MINUS_ONE), (MINUS_ONE, MINUS_ONE), (MINUS_ONE, jm.IDENTITY), (jm.add(P, MINUS_ONE), jm.add(P, MINUS_ONE))]
    for a, b in cases:
        assert lib_add(jj, a, b) == jm.point_words(jm.add(a, b)), (a, b)
    assert lib_add(jj, P, jm.neg(P)) == jm.point_words(jm.IDENTITY)
    assert lib_add(jj, MINUS_ONE, MINUS_ONE) == jm.point_words(jm.IDENTITY)
    for a in (P, Q, jm.IDENTITY, MINUS_ONE, jm.uncleared_point()):
        out = np.zeros(8, np.uint64)
        jj.chk_jj_dbl(p(pt(a)), p(out))
        assert out.tolist() == jm.point_words(jm.add(a, a))


def test_mixed_addition_with_an_entry_and_with_its_negative(jj, gens):
    P, Q = gens[0], gens[2]
    for a, b in [(P, Q), (P, P), (jm.IDENTITY, Q), (jm.neg(Q), Q), (MINUS_ONE, Q), (jm.mul(Q, 5), Q)]:
        for negative in (0, 1):
            out = np.zeros(8, np.uint64)
            jj.chk_jj_madd(p(pt(a)), p(pt(b)), negative, p(out))
            assert out.tolist() == jm.point_words(jm.add(a, jm.neg(b) if negative else b)), (a, b, negative)


def test_all_eight_chunk_encodings(jj):
    for s0 in (0, 1):
        for s1 in (0, 1):
            for s2 in (0, 1):
                assert jj.chk_jj_encode(s0, s1, s2) == jm.encode((s0, s1, s2)) == (1 - 2 * s2) * (1 + s0 + 2 * s1)
    assert sorted(jm.encode((a, b, c)) for a in (0, 1) for b in (0, 1) for c in (0, 1)) == [-4, -3, -2, -1, 1, 2, 3, 4]


def test_schedule_of_segments_and_windows(jj):
    assert jj.chk_jj_max_bits(G) == 189 * G
    for n in SIZES:
        seg = np.zeros(200, np.uint32); win = np.zeros(200, np.uint32)
        count = jj.chk_jj_schedule(n, p(seg), p(win))
        assert count == (n + 2) // 3
        assert list(zip(seg[:count].tolist(), win[:count].tolist())) == jm.schedule(n)
        assert all(w < 63 for w in win[:count]) and seg[count - 1] == (count - 1) // 63


def test_table_windows_from_the_generator_equal_the_running_ones(jj, table):
    t, ga = table
    for i in range(G):
        for j in (0, 1, 31, 62):
            assert jj.chk_jj_table_window(t, p(ga), i, j) == 1


def lib_hash(jj, t, bits, lanes=1, words=None, counters=False):
    n = len(bits)
    w = np.array(jm.message_words(bits) if words is None else words, np.uint64)
    digest = np.zeros(4, np.uint64); point = np.zeros(8, np.uint64)
    added = np.zeros((n + 2) // 3, np.uint32); gave = np.zeros(lanes, np.uint32)
    assert jj.chk_jj_hash(t, p(w), n, 0, lanes, p(digest), p(point), p(added), p(gave)) == 0
    return (digest.tolist(), point.tolist(), added, gave) if counters else (digest.tolist(), point.tolist())


def test_hash_against_both_routes_of_the_model(jj, table, gens, model):
    t, _ = table
    rng = random.Random(11)
    for n in SIZES:
        for bits in ([rng.getrandbits(1) for _ in range(n)], [0] * n, [1] * n):
            want = model.hash_point(bits)
            assert jm.hash_definition(gens, bits) == want           # the definition's route (slow) agrees on every case
            digest, point = lib_hash(jj, t, bits)
            assert digest == jm.words(want[0]) and point == jm.point_words(want)
    assert jm.hash_definition(gens, [1] * 567) == model.hash_point([1] * 567)


def test_stray_bits_above_n_are_ignored(jj, table, model):
    t, _ = table
    rng = random.Random(12)
    for n in (1, 3, 4, 63, 64, 65, 190, 255, 510):
        bits = [rng.getrandbits(1) for _ in range(n)]
        clean = jm.message_words(bits)
        dirty = list(clean)
        dirty[-1] |= (0xFFFFFFFFFFFFFFFF << (n % 64)) & 0xFFFFFFFFFFFFFFFF if n % 64 else 0
        if n % 64:
            assert dirty != clean
        assert lib_hash(jj, t, bits, words=dirty)[0] == jm.words(model.hash(bits))
        w = np.array(dirty, np.uint64)
        assert [jj.chk_jj_message_bit(p(w), n, 0, k) for k in range(n + 3)] == bits + [0, 0, 0]


def test_lane_shares_and_fold_order(jj, table, model):
    t, _ = table
    rng = random.Random(13)
    for n in SIZES:
        bits = [rng.getrandbits(1) for _ in range(n)]
        want = jm.words(model.hash(bits))
        for lanes in LANES:
            digest, _, added, gave = lib_hash(jj, t, bits, lanes, counters=True)
            assert digest == want, (n, lanes)
            assert (added == 1).all(), (n, lanes)                    # every chunk is added exactly once
            assert (gave <= 1).all() and gave.sum() == lanes - 1     # every lane but lane 0 gives once
    for lanes in LANES:
        levels = [s for s in (32, 16, 8, 4, 2, 1) if s < lanes]
        for lane in range(lanes):
            role = [jj.chk_jj_fold(lane, lanes, s) for s in (32, 16, 8, 4, 2, 1)]
            assert sum(1 for r in role if r & 1) == (0 if lane == 0 else 1)
            assert not any(r == 3 for r in role)
        assert [jj.chk_jj_fold(0, lanes, s) for s in levels] == [2] * len(levels)
    assert [jj.chk_jj_group_lanes(c) for c in (1, 2047, 2048, 8191, 8192, 65535, 65536, 1 << 24)] == [64, 64, 16, 16, 4, 4, 1, 1]


def test_coinciding_and_cancelling_partial_sums(jj, gens):
    """generators G_1 = G_0: a 378-bit message whose second segment repeats the first doubles inside the fold; with every s2 of the
    second segment flipped the sum is the identity"""
    same = [gens[0], gens[0]]
    ga = np.array([jm.point_words(g) for g in same], np.uint64)
    t = C.c_void_p(jj.chk_jj_table_new(p(ga), 2))
    rng = random.Random(14)
    first = [rng.getrandbits(1) for _ in range(189)]
    flipped = [b ^ 1 if k % 3 == 2 else b for k, b in enumerate(first)]
    twice = jm.Table(same).hash_point(first + first)
    assert twice == jm.add(jm.Table(same).hash_point(first), jm.Table(same).hash_point(first))
    for lanes in LANES:
        assert lib_hash(jj, t, first + first, lanes)[1] == jm.point_words(twice)
        assert lib_hash(jj, t, first + flipped, lanes) == ([0, 0, 0, 0], jm.point_words(jm.IDENTITY))
    jj.chk_jj_table_free(t)


def test_generator_tests_reject_what_they_must(jj, gens):
    raw = jm.uncleared_point()
    assert jm.on_curve(raw) and not jm.has_order_s(raw)
    off = (gens[0][0], (gens[0][1] + 1) % jm.R)
    big_u = np.array(jm.words(gens[0][0] + jm.R) + jm.words(gens[0][1]), np.uint64)
    big_v = np.array(jm.words(0) + jm.words(jm.R), np.uint64)
    assert jj.chk_jj_generator_fault(p(pt(gens[0]))) == 0 and jj.chk_jj_generator_fault(p(pt(jm.neg(gens[1])))) == 0
    assert jj.chk_jj_generator_fault(p(big_u)) == 1 and jj.chk_jj_generator_fault(p(big_v)) == 1
    assert jj.chk_jj_generator_fault(p(pt(off))) == 2
    assert jj.chk_jj_generator_fault(p(pt(jm.IDENTITY))) == 3
    assert jj.chk_jj_generator_fault(p(pt(MINUS_ONE))) == 4
    assert jj.chk_jj_generator_fault(p(pt(raw))) == 4
    assert jj.chk_jj_on_curve(p(pt(raw))) == 1 and jj.chk_jj_prime_order(p(pt(raw))) == 0
    assert jj.chk_jj_on_curve(p(pt(MINUS_ONE))) == 1 and jj.chk_jj_prime_order(p(pt(MINUS_ONE))) == 0
    assert jj.chk_jj_on_curve(p(pt(jm.IDENTITY))) == 1 and jj.chk_jj_prime_order(p(pt(jm.IDENTITY))) == 0
    assert jj.chk_jj_on_curve(p(pt(off))) == 0 and jj.chk_jj_on_curve(p(big_u)) == 0
    for g in gens:
        assert jj.chk_jj_on_curve(p(pt(g))) == 1 and jj.chk_jj_prime_order(p(pt(g))) == 1


def test_blob_bit_order_and_rt_split(jj):
    digest = sum(1 << b for b in (0, 7, 8, 253, 254))
    d = np.array(jm.words(digest), np.uint64)
    blob = np.zeros(32, np.uint8)
    jj.chk_jj_blob(p(d), p(blob))
    assert blob.tobytes() == jm.node_blob(digest)
    assert blob[0] == 0x81 and blob[1] == 0x80 and blob[31] == 0x06 and not blob[2:31].any()
    back = np.zeros(4, np.uint64)
    jj.chk_jj_unblob(p(blob), p(back))
    assert back.tolist() == d.tolist()
    rt = np.zeros(8, np.uint64)
    jj.chk_jj_rt_split(p(d), p(rt))
    assert rt.tolist() == jm.words(jm.rt_scalars(digest)[0]) + jm.words(jm.rt_scalars(digest)[1])
    assert jm.rt_scalars(digest) == [digest - (1 << 254), 1]
    for depth, level, first in ((0, 0, 0), (3, 0, 0), (3, 1, 8), (3, 3, 14), (9, 9, 1022)):
        assert jj.chk_jj_level_first(depth, level) == first
    assert [jj.chk_jj_sibling(5, l) for l in range(3)] == [4, 3, 0]


def test_small_trees_against_the_model(jj, table, model):
    t, _ = table
    rng = random.Random(15)
    for depth, count, hash_leaves in ((0, 1, 1), (0, 0, 0), (1, 2, 1), (2, 3, 1), (2, 4, 0), (3, 5, 1)):
        keys = [rng.getrandbits(255) for _ in range(count)]
        pks = np.array([jm.words(k) for k in keys] + [[0, 0, 0, 0]], np.uint64)
        nodes = np.zeros(((2 << depth) - 1, 4), np.uint64)
        assert jj.chk_jj_tree(t, p(pks), count, depth, hash_leaves, p(nodes)) == 0
        levels = model.tree(keys, depth, bool(hash_leaves))
        assert nodes.tolist() == [jm.words(n) for level in levels for n in level]
        for x in range(1 << depth):
            assert jm.copath(levels, x) == [levels[l][jj.chk_jj_sibling(x, l)] for l in range(depth)]


def test_stand_alone_program_under_sanitizers(tmp_path):
    """jubjub_check.cpp with its own main under AddressSanitizer and UBSan: no code loaded into python"""
    exe = str(tmp_path / "jubjub_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DJUBJUB_CHECK_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "jubjub_check: ok" in r.stdout, r.stdout + r.stderr
