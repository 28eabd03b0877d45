"""CPU build of the ballot box's rules: vote_saver_protocol_amd/csrc/ballot_box.h compiled by g++.  The claim and resolve steps that
k_box_claim and k_box_resolve run are executed one slot operation at a time under many interleavings of the lanes (fixed seeds) and
compared with a Python dict walked in index order -- "the lowest index wins" --; chains, the wrap around the table's end, a table at
exactly half load and a full table that must end the probe at its bound come from serials searched for their hash.  No GPU."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpu_build", "ballot_box_check.cpp")
EMPTY = NONE = (1 << 64) - 1
PENDING = 1 << 63
SEEDS = range(1, 25)


@pytest.fixture(scope="module")
def bb(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cpu_build") / "libboxchk.so")
    flags = os.environ.get("VSP_MATHCHK_FLAGS", "-O2").split()
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.chk_box_hash.restype = C.c_uint32
    lib.chk_box_hash.argtypes = [C.c_void_p, C.c_size_t]
    lib.chk_box_probe.restype = C.c_uint64
    lib.chk_box_probe.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64]
    lib.chk_box_slots_for.restype = C.c_uint64
    lib.chk_box_slots_for.argtypes = [C.c_uint, C.c_uint64]
    lib.chk_box_piece.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.chk_box_find.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.chk_box_rebuild.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64]
    lib.chk_box_fixed_match.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.chk_box_gather_serial.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    return lib


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def hash_of(lib, serial):
    return lib.chk_box_hash(p(serial), serial.shape[0])


def serial_with_home(lib, rng, words, slots, home):
    """a random serial whose first probe is slot `home`"""
    while True:
        s = np.array([rng.getrandbits(32) for _ in range(words)], np.uint32)
        if hash_of(lib, s) & (slots - 1) == home:
            return s


def run_piece(lib, table, store, pend, skip, seed):
    c, words = pend.shape
    win = np.zeros(c, np.uint64); pos = np.zeros(c, np.uint64); steps = C.c_uint64(0)
    flag = lib.chk_box_piece(p(table), table.shape[0], p(store), p(pend), words, p(skip), c, seed, p(win), p(pos), C.byref(steps))
    return flag, win, pos, steps.value


def model(committed, pend, skip):
    """the dict walked in index order -> per lane the slot value it must read: its own pending value when it wins, the winner's
    pending value, or the committed ordinal"""
    held = {bytes(s.tobytes()): o for o, s in enumerate(committed)}
    want = []
    for k in range(pend.shape[0]):
        if skip[k]:
            want.append(NONE)
            continue
        key = bytes(pend[k].tobytes())
        if key not in held:
            held[key] = PENDING | k
        want.append(held[key])
    return want


def check_piece(lib, bits, committed, pend, skip=None, seeds=SEEDS):
    """claims and resolves under every seed; the winners against the model, every slot's key unique, the table otherwise untouched"""
    slots, words = 1 << bits, pend.shape[1]
    skip = np.zeros(pend.shape[0], np.uint8) if skip is None else skip
    store = np.concatenate([committed.reshape(-1), np.zeros(words, np.uint32)]).reshape(-1, words)
    base = np.full(slots, EMPTY, np.uint64)
    if committed.shape[0]:
        assert lib.chk_box_rebuild(p(base), slots, p(store), words, committed.shape[0], 1) == 0
    want = model(committed, pend, skip)
    longest = 0
    for seed in seeds:
        table = base.copy()
        flag, win, pos, steps = run_piece(lib, table, store, pend, skip, seed)
        assert flag == 0, (seed, flag)
        assert win.tolist() == want, seed
        longest = max(longest, steps)
        # what the table holds afterwards: the committed ordinals and one pending value per new key, the winner's
        values = sorted(int(x) for x in table if x != EMPTY)
        assert values == sorted(set(range(committed.shape[0])) | {w for w in want if w != NONE and w & PENDING}), seed
        for k in range(pend.shape[0]):
            if not skip[k]:
                assert int(table[int(pos[k])]) == want[k]
    return longest


def random_serials(rng, count, words):
    return np.array([[rng.getrandbits(32) for _ in range(words)] for _ in range(count)], np.uint32).reshape(count, words)


@pytest.mark.parametrize("S", [1, 2, 8])
@pytest.mark.parametrize("bits", [2, 3, 4])
def test_lowest_index_wins_under_every_interleaving(bb, bits, S):
    rng = random.Random(100 * bits + S)
    words, slots = 8 * S, 1 << bits
    none = np.zeros((0, words), np.uint32)
    c = slots // 2                                                   # with distinct serials: exactly half load
    distinct = random_serials(rng, c, words)
    check_piece(bb, bits, none, distinct)
    # equal serials at indices 0 and c - 1
    ends = distinct.copy(); ends[c - 1] = ends[0]
    check_piece(bb, bits, none, ends)
    # every lane the same serial, more lanes than slots
    same = np.repeat(random_serials(rng, 1, words), 2 * slots + 1, axis=0)
    check_piece(bb, bits, none, same)
    # a serial five times among others, and lanes that do not take part (verdict 0) holding the lowest index of a key
    mixed = random_serials(rng, c, words)
    if c >= 2:
        mixed = np.concatenate([mixed[:1], mixed[:1], mixed[1:2], mixed[:1], mixed[:1], mixed[:1]])[:max(c, 2) + 4]
        skip = np.zeros(mixed.shape[0], np.uint8); skip[0] = 1
        check_piece(bb, bits, none, mixed, skip)


@pytest.mark.parametrize("S", [1, 2, 8])
@pytest.mark.parametrize("bits", [2, 3, 4])
def test_one_probe_chain_around_the_tables_end(bb, bits, S):
    """every serial hashes to the last slot: the chain wraps to slot 0 and the lanes contend for every slot of it"""
    rng = random.Random(200 * bits + S)
    words, slots = 8 * S, 1 << bits
    c = slots // 2
    chain = np.array([serial_with_home(bb, rng, words, slots, slots - 1) for _ in range(c)], np.uint32).reshape(c, words)
    assert all(bb.chk_box_probe(hash_of(bb, s), 1, slots) == 0 for s in chain)
    none = np.zeros((0, words), np.uint32)
    longest = check_piece(bb, bits, none, chain)
    assert longest <= c + 1                                          # at most the chain and one minimum
    # with repeats inside the chain
    rep = np.concatenate([chain, chain[::-1]])
    check_piece(bb, bits, none, rep)
    # against committed serials of the same chain: a committed holder stays, whatever claims
    if c >= 2:
        committed = chain[:c // 2]
        pend = np.concatenate([chain[c // 2:], committed, chain[c // 2:]])
        check_piece(bb, bits + 1, committed, pend)


def test_committed_serials_are_found_and_absent_ones_end_at_an_empty_slot(bb):
    rng = random.Random(7)
    words, bits = 16, 4
    slots = 1 << bits
    committed = random_serials(rng, 8, words)                       # exactly half load
    table = np.zeros(slots, np.uint64)
    for seed in range(1, 6):
        assert bb.chk_box_rebuild(p(table), slots, p(committed), words, 8, seed) == 0
        assert sorted(int(x) for x in table if x != EMPTY) == list(range(8))
        for o in range(8):
            v = C.c_uint64(0)
            assert bb.chk_box_find(p(table), slots, p(committed), p(committed), words, p(committed[o]), C.byref(v)) == 1 and v.value == o
        for other in random_serials(rng, 20, words):
            v = C.c_uint64(0)
            assert bb.chk_box_find(p(table), slots, p(committed), p(committed), words, p(other), C.byref(v)) == 0


@pytest.mark.parametrize("bits", [2, 3, 4])
def test_a_probe_ends_at_the_bound_and_raises_the_flag(bb, bits):
    """a table without an empty slot (growth keeps a real one half empty): claim and find take `slots` steps, report, and stop"""
    rng = random.Random(300 + bits)
    words, slots = 8, 1 << bits
    store = random_serials(rng, slots, words)
    table = np.arange(slots, dtype=np.uint64)                        # every slot a committed ordinal of another key
    pend = random_serials(rng, 3, words)
    before = table.copy()
    flag, win, pos, steps = run_piece(bb, table, store, pend, np.zeros(3, np.uint8), 5)
    assert flag == 1 and steps == slots and win.tolist() == [NONE] * 3
    assert np.array_equal(table, before)
    v = C.c_uint64(0)
    assert bb.chk_box_find(p(table), slots, p(store), p(pend), words, p(pend[0]), C.byref(v)) == -1
    # the rebuild of more serials than slots reports as well
    assert bb.chk_box_rebuild(p(table), slots, p(np.concatenate([store, pend])), words, slots + 3, 1) == 1


def test_growth_keeps_the_table_at_most_half_full(bb):
    for bits in (2, 3, 16):
        for held in (0, 1, (1 << bits) // 2, (1 << bits) // 2 + 1, 1 << bits, 5 << bits):
            slots = bb.chk_box_slots_for(bits, held)
            assert slots >= 1 << bits and slots & (slots - 1) == 0 and 2 * held <= slots
            assert slots == 1 << bits or 2 * held > slots // 2      # the smallest such table


def test_roles_select_the_fixed_inputs_and_the_serial(bb):
    rng = random.Random(9)
    L = 5
    rest = random_serials(rng, L, 8)
    role = np.array([1, 2, 2, 1, 0], np.uint8)
    out = np.zeros(16, np.uint32)
    bb.chk_box_gather_serial(p(rest), p(role), L, p(out))
    assert np.array_equal(out, np.concatenate([rest[1], rest[2]]))
    expected = rest.copy()
    expected[1] ^= 1; expected[4] ^= 1                               # SERIAL and FREE inputs are not compared
    assert bb.chk_box_fixed_match(p(rest), p(expected), p(role), L) == 1
    for i, word in ((0, 0), (0, 7), (3, 4)):
        bad = expected.copy(); bad[i, word] ^= 0x80000000
        assert bb.chk_box_fixed_match(p(rest), p(bad), p(role), L) == 0
    # the hash depends on every word and on the length
    base = random_serials(rng, 1, 16)[0]
    h = hash_of(bb, base)
    for i in range(16):
        t = base.copy(); t[i] ^= 1
        assert hash_of(bb, t) != h
    assert bb.chk_box_hash(p(base), 8) != bb.chk_box_hash(p(np.concatenate([base[:8], np.zeros(8, np.uint32)])), 16)


def test_stand_alone_program_under_sanitizers(tmp_path):
    """ballot_box_check.cpp with its own main under AddressSanitizer and UBSan: no code loaded into python"""
    exe = str(tmp_path / "ballot_box_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DBALLOT_BOX_CHECK_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ballot_box_check: ok" in r.stdout, r.stdout + r.stderr
