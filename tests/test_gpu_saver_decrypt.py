"""GPU: vsp_saver_decrypt_batch and vsp_saver_verify_decryption_batch -- the tally opened and a published result checked.  Keys and
ciphertexts come from tests/dlog_decrypt.py (every point a known multiple of a generator, so the expected message, status and reason
of every member are known without a pairing); one test runs a real key end to end and asks oracle/saver.py."""
import contextlib

import numpy as np
import pytest

import bls12_381 as o
import saver as sv
from conftest import I, L, fr_array, g1_limbs

import dlog_decrypt as dd
from dlog_election import g1_points, g2_points, rng as make_rng

import vote_saver_protocol_amd as v

pytestmark = pytest.mark.gpu
R, NONE = o.R, dd.NONE
NO_SLOT = 0xFFFFFFFF


@contextlib.contextmanager
def decryptor(ctx, key, max_value, baby_bits=0, fp_bits=64):
    """a SaverDecryptor made under the two options (SaverDecryptor sets them for its creation alone and puts them back)"""
    dec = v.SaverDecryptor(ctx, key.vk_words, key.gamma_abc, key.n, max_value, baby_bits=baby_bits, fp_bits=fp_bits)
    try:
        yield dec
    finally:
        dec.free()


def decrypt(ctx, dec, key, members):
    """(msgs, status) as lists of rows, after checking nu against the model's rho u_0"""
    msgs, nu, status = v.saver_decrypt_batch(ctx, dec, key.rho_limbs, dd.ct_batch(key, members))
    assert np.array_equal(nu, g1_points([key.rho * us[0] for us in members]))
    return msgs.tolist(), status.tolist()


def check_against_model(ctx, dec, key, members, max_value):
    msgs, status = decrypt(ctx, dec, key, members)
    want = [key.decrypt(us, max_value) for us in members]
    assert msgs == [w[0] for w in want] and status == [w[1] for w in want]
    return msgs, status


def test_search_boundaries_with_eight_baby_steps(ctx):
    """msg_size 3, B = 8, max_value 100: 13 giant steps reach 103; r - 1 is the log of a ciphertext built for -1"""
    rg = make_rng(1)
    key = dd.DecryptKey(rg, 3)
    found, lost = [0, 1, 7, 8, 9, 63, 64, 96, 100], [101, 103, 104, R - 1]
    with decryptor(ctx, key, 100, baby_bits=3) as dec:
        assert dec.baby_bits == 3 and dec.max_value == 100 and ctx.lib.vsp_saver_decryptor_msg_size(dec.h) == 3
        members = [key.ciphertext([m, found[(k + 1) % len(found)], 0], rg) for k, m in enumerate(found)]
        members += [key.ciphertext([5, m, 100], rg) for m in lost]
        msgs, status = check_against_model(ctx, dec, key, members, 100)
        assert [row[0] for row in msgs[:len(found)]] == found and all(s == [0, 0, 0] for s in status[:len(found)])
        assert msgs[len(found):] == [[5, NONE, 100]] * len(lost) and status[len(found):] == [[0, 1, 0]] * len(lost)


def test_lane_run_and_block_boundaries_and_a_partial_last_block(ctx):
    """msg_size 1, B = 2, max_value 2^14 + 5: 8 195 giant steps, so with S giant steps a lane and L lanes a block (the constants the
    library states) 129 lanes in two full blocks and one lane more.  A message on each side of every lane-run boundary (multiples
    of 2 S) -- the block boundaries (multiples of 2 S L) are among them"""
    S, Lb = int(ctx.stat("saver_decrypt_run_steps")), int(ctx.stat("saver_decrypt_block_lanes"))
    assert S >= 1 and Lb >= 1
    max_value = (1 << 14) + 5
    giants = (max_value >> 1) + 1
    assert giants == 8195
    lanes = -(-giants // S)
    assert lanes > 2 * Lb and lanes % Lb, "the shape is meant to fill several blocks and leave the last one partial"
    edges = [k * 2 * S for k in range(1, lanes)]
    assert any(e % (2 * S * Lb) == 0 for e in edges)
    want = sorted({0, 1, max_value, max_value + 1} | {e - 1 for e in edges} | set(edges))
    rg = make_rng(2)
    key = dd.DecryptKey(rg, 1)
    with decryptor(ctx, key, max_value, baby_bits=1) as dec:
        msgs, status = check_against_model(ctx, dec, key, [key.ciphertext([m], rg) for m in want], max_value)
        assert [row[0] for row in msgs] == want[:-1] + [NONE] and [row[0] for row in status] == [0] * (len(want) - 1) + [1]


def test_the_giant_range_in_several_launches_and_the_early_stop(ctx):
    """msg_size 2, B = 2, max_value 2^14 + 5 with 260 ciphertexts: 520 items leave every item one block of lanes a launch (the rule
    and its constants are the library's: max(L, floor(launch_lanes / items / L) L)), so the 129 lanes of an item's range take three
    launches -- 64, 64 and 1 lanes.  Counts on each side of both launch boundaries and in the last launch; the number of launches,
    which the library counts, is 3 when one slot has no count in range, and 1, 2, 3 when the largest count lies in the first, second,
    third launch: the search stops as soon as no item is pending, and not before"""
    S, Lb, LL = (int(ctx.stat("saver_decrypt_" + k)) for k in ("run_steps", "block_lanes", "launch_lanes"))
    max_value, count, n = (1 << 14) + 5, 260, 2
    runs = -(-((max_value >> 1) + 1) // S)
    lanes = min(runs, max(Lb, LL // (count * n) // Lb * Lb))
    launches = -(-runs // lanes)
    assert (S, Lb, lanes, launches) == (64, 64, 64, 3), "the shape is meant to need three launches, the last a single lane"
    edge = [k * lanes * S * 2 for k in range(1, launches)]            # the first count of launch k: lane k * lanes, B = 2
    assert edge == [8192, 16384] and edge[-1] <= max_value
    rg = make_rng(12)
    key = dd.DecryptKey(rg, n)
    near = [0, 1, edge[0] - 1, edge[0], edge[0] + 1, edge[1] - 1, edge[1], edge[1] + 1, max_value]

    def batch(top, lost=False):
        """260 ciphertexts with counts below `top`, the boundary counts below `top` among them, the largest top - 1; lost: one slot
        out of range"""
        rows = [[rg.randrange(top), rg.randrange(top)] for _ in range(count)]
        for k, m in enumerate(x for x in near if x < top):
            rows[7 * k + 3][k % 2] = m
        rows[count - 1][1] = top - 1
        if lost:
            rows[100][0] = max_value + 1
        return rows

    with decryptor(ctx, key, max_value, baby_bits=1) as dec:
        for top, lost, want_launches in ((max_value + 1, True, 3), (edge[0], False, 1), (edge[1], False, 2), (max_value + 1, False, 3), (40, False, 1)):
            rows = batch(top, lost)
            ctx.stats_reset()
            msgs, status = check_against_model(ctx, dec, key, [key.ciphertext(row, rg) for row in rows], max_value)
            assert ctx.stat("saver_decrypt_dlog_launches") == want_launches, (top, lost)
            if lost:
                rows[100][0] = NONE
            assert msgs == rows and [s for row in status for s in row].count(1) == int(lost)
        assert ctx.stat("saver_decrypt_launch_lanes") == LL                 # a constant: the reset above did not touch it


def test_creation_puts_the_two_options_back(ctx):
    rg = make_rng(13)
    key = dd.DecryptKey(rg, 1)
    try:
        ctx.set_option("saver_decrypt_baby_bits", 2)
        with v.SaverDecryptor(ctx, key.vk_words, key.gamma_abc, 1, 1000, baby_bits=4, fp_bits=7) as forced:
            assert forced.baby_bits == 4
        with v.SaverDecryptor(ctx, key.vk_words, key.gamma_abc, 1, 1000) as later:      # the context's own 2, and 64-bit fingerprints again
            assert later.baby_bits == 2 and ctx.options["saver_decrypt_baby_bits"] == 2 and ctx.options["saver_decrypt_fp_bits"] == 64
        with pytest.raises(v.VspError, match=r"2\^24"):                                  # a refused creation puts them back too
            v.SaverDecryptor(ctx, key.vk_words, key.gamma_abc, 1, 1 << 40, baby_bits=1)
        assert ctx.options["saver_decrypt_baby_bits"] == 2
    finally:
        ctx.set_option("saver_decrypt_baby_bits", 0)
    with v.SaverDecryptor(ctx, key.vk_words, key.gamma_abc, 1, 1000) as dec:
        assert dec.baby_bits == 5


def test_automatic_baby_bits_for_a_32_bit_range(ctx):
    rg = make_rng(3)
    key = dd.DecryptKey(rg, 2)
    want = [(1 << 32) - 1, (1 << 31) + 12345, 65535, 65536, 0]
    with decryptor(ctx, key, (1 << 32) - 1) as dec:
        assert dec.baby_bits == 16 and ctx.lib.vsp_saver_decryptor_baby_bits(dec.h) == 16
        members = [key.ciphertext([m, want[(k + 2) % 5]], rg) for k, m in enumerate(want)]
        msgs, status = check_against_model(ctx, dec, key, members, (1 << 32) - 1)
        assert [row[0] for row in msgs] == want and status == [[0, 0]] * 5


def test_collision_path_with_a_four_bit_fingerprint(ctx):
    """64 baby steps under 16 fingerprints: every lookup meets about four table entries, each tried and confirmed.  Every m in 0..255
    over 4 slots x 64 ciphertexts, each slot in another order"""
    rg = make_rng(4)
    key = dd.DecryptKey(rg, 4)
    with decryptor(ctx, key, 255, baby_bits=6, fp_bits=4) as dec:
        rows = [[(4 * k + i) * (2 * i + 1) % 256 for i in range(4)] for k in range(64)]
        assert {m for row in rows for m in row} == set(range(256))
        msgs, status = check_against_model(ctx, dec, key, [key.ciphertext(row, rg) for row in rows], 255)
        assert msgs == rows and status == [[0] * 4] * 64


@pytest.mark.parametrize("n", [1, 2, 25, 64])
def test_shapes_with_one_slot_out_of_range_per_ciphertext(ctx, n):
    """66 ciphertexts: one full wave and two lanes.  Mixed messages; slot k mod n of ciphertext k is out of range, and only it"""
    rg = make_rng(50 + n)
    key = dd.DecryptKey(rg, n)
    max_value = 1000
    rows = [[rg.randrange(max_value + 1) if i != k % n else max_value + 1 + rg.randrange(5000) for i in range(n)] for k in range(66)]
    with decryptor(ctx, key, max_value) as dec:
        assert dec.baby_bits == 5
        msgs, status = check_against_model(ctx, dec, key, [key.ciphertext(row, rg) for row in rows], max_value)
        assert status == [[1 if i == k % n else 0 for i in range(n)] for k in range(66)]
        assert msgs == [[NONE if i == k % n else rows[k][i] for i in range(n)] for k in range(66)]
        try:                                                          # the same in pieces of 20, 20, 20, 6
            ctx.set_option("pairing_chunk", 20)
            again, st2 = decrypt(ctx, dec, key, [key.ciphertext(row, rg) for row in rows])
            assert again == msgs and st2 == status
        finally:
            ctx.set_option("pairing_chunk", 1 << 14)


def test_exceptional_members(ctx):
    rg = make_rng(6)
    key = dd.DecryptKey(rg, 3)
    max_value = 500
    with decryptor(ctx, key, max_value) as dec:
        plain = key.ciphertext([3, 4, 5], rg)
        c0_inf = [0, key.member(0, 7, 0), key.member(1, 0, 0), key.member(2, 500, 0), rg.randrange(1, R)]       # c_0 = infinity: nu = infinity
        empty = [0] * 5                                                                                   # an empty tally
        ci_inf = key.ciphertext([1, 2, 3], rg); ci_inf[2] = 0                                             # c_2 = infinity beside a real c_0
        equal = key.ciphertext([9, 9, 9], rg); equal[2] = equal[1]                                        # c_2 = c_1
        members = [plain, c0_inf, empty, ci_inf, equal, plain]
        assert key.member(1, 0, 0) == 0 and key.decrypt(c0_inf, max_value) == ([7, 0, 500], [0, 0, 0])
        assert key.decrypt(empty, max_value) == ([0, 0, 0], [0, 0, 0])
        assert key.decrypt(ci_inf, max_value)[1][1] == 1                                                  # by the equations: no small message
        msgs, status = check_against_model(ctx, dec, key, members, max_value)
        assert msgs[0] == [3, 4, 5] and msgs[5] == [3, 4, 5] and msgs[4][0] == 9 and msgs[4][2] == 9
        # malformed members: status 2 for that ciphertext alone
        ct = dd.ct_batch(key, members)
        ct[1, 1, 6] ^= np.uint64(1)                                                                       # c_1 off the curve
        ct[3, 0, :6] = L(o.P, 6)                                                                          # a coordinate equal to p
        got, nu, st = v.saver_decrypt_batch(ctx, dec, key.rho_limbs, ct)
        want = [key.decrypt(us, max_value) for us in members]
        for k in range(6):
            if k in (1, 3):
                assert st[k].tolist() == [2, 2, 2] and got[k].tolist() == [NONE] * 3 and not nu[k].any()
            else:
                assert got[k].tolist() == want[k][0] and st[k].tolist() == want[k][1]
        # psi takes no part: a psi off the curve changes nothing
        ct = dd.ct_batch(key, [plain]); ct[0, 4, 6] ^= np.uint64(1)
        got, _, st = v.saver_decrypt_batch(ctx, dec, key.rho_limbs, ct)
        assert got.tolist() == [[3, 4, 5]] and st.tolist() == [[0, 0, 0]]


def test_nu_is_the_oracles_multiple_limb_for_limb(ctx):
    rg = make_rng(7)
    key = dd.DecryptKey(rg, 1)
    us = key.ciphertext([1], rg)
    ct = dd.ct_batch(key, [us, [0, 0, 0]])
    c0 = o.g1_from_limbs(ct[0, 0])
    with decryptor(ctx, key, 10) as dec:
        for rho in (1, R - 1, rg.randrange(1, R)):
            _, nu, _ = v.saver_decrypt_batch(ctx, dec, fr_array([rho])[0], ct)
            assert np.array_equal(nu[0], g1_limbs(o.G1.mul(c0, rho))), rho
            assert not nu[1].any()                                     # c_0 = infinity


def test_verify_decryption_verdicts(ctx):
    rg = make_rng(8)
    key = dd.DecryptKey(rg, 3)
    G = 1
    with decryptor(ctx, key, 100, baby_bits=3) as dec:
        base = [key.ciphertext([rg.randrange(101) for _ in range(3)], rg) for _ in range(5)]
        minus_one = key.ciphertext([R - 1, 2, 3], rg)                                        # built for -1
        cases = []                                                                           # (ciphertext logs, msgs, nu log)
        for us in base:
            true = [key.slot_log(us, i) for i in range(3)]
            nu = key.rho * us[0] % R
            cases.append((us, true, nu))                                                     # the true result
            cases.append((us, [true[0], true[1] + 1, true[2]], nu))                          # one message off by one
            cases.append((us, [true[0], (true[1] - 1) % R, true[2] + 1], nu))                # two wrong slots
            cases.append((us, true, (nu + G) % R))                                           # nu + G
        cases.append((minus_one, [R - 1, 2, 3], key.rho * minus_one[0] % R))                 # a full-width power
        cases.append((minus_one, [R, 2, 3], key.rho * minus_one[0] % R))                     # m = r: malformed
        cases.append((minus_one, [R - 1, 2, (1 << 256) - 1], key.rho * minus_one[0] % R))
        want = [key.reason(us, m, nu) for us, m, nu in cases]
        assert [w[0] for w in want[:4]] == [0, 4, 4, 6] and [w[1] for w in want[:4]] == [NO_SLOT, 1, 1, 0]
        assert [w[0] for w in want[-3:]] == [0, 1, 1]
        ct = dd.ct_batch(key, [c[0] for c in cases])
        msgs = dd.scalars([c[1] for c in cases])
        nus = g1_points([c[2] for c in cases])
        verdict, reason, first = v.saver_verify_decryption_batch(ctx, dec, ct, msgs, nus)
        assert reason.tolist() == [w[0] for w in want] and first.tolist() == [w[1] for w in want]
        assert verdict.tolist() == [int(w[0] == 0) for w in want]
        # malformed points: reason 1 for that member alone
        ct2, nus2 = ct.copy(), nus.copy()
        ct2[0, 1, 6] ^= np.uint64(1)
        nus2[4, 6:] = L(o.P, 6)
        verdict, reason, first = v.saver_verify_decryption_batch(ctx, dec, ct2, msgs, nus2)
        assert reason.tolist() == [1 if k in (0, 4) else w[0] for k, w in enumerate(want)]
        assert first.tolist() == [NO_SLOT if k in (0, 4) else w[1] for k, w in enumerate(want)]
        # what decrypt returns is accepted
        got, nu, st = v.saver_decrypt_batch(ctx, dec, key.rho_limbs, dd.ct_batch(key, base))
        assert not st.any()
        verdict, reason, _ = v.saver_verify_decryption_batch(ctx, dec, dd.ct_batch(key, base), got, nu)
        assert verdict.tolist() == [1] * 5 and reason.tolist() == [0] * 5


def test_real_key_end_to_end_with_the_oracle(ctx, cref):
    """msg_size 2: a key of saver_generate_keypair, three ballots and one large ciphertext encrypted by the C oracle, added through
    Tally from blobs, opened on the GPU; oracle/saver.py verify_decryption judges the GPU's result and a tampered one"""
    n = 2
    gen = o.splitmix64(99)
    pts = g1_points([o.rand_fr(gen) for _ in range(n + 3)])
    gabc, delta_g1, gamma_g1 = np.ascontiguousarray(pts[:n + 1]), pts[n + 1], pts[n + 2]
    rnd = fr_array([o.rand_fr(gen) for _ in range(3 * n + 2)])
    pk_w, sk, vk_w = v.saver_generate_keypair(ctx, rnd, gabc, delta_g1, gamma_g1, n)
    ballots = [[1, 0], [0, 1], [1, 0], [70000, 0]]
    tally = v.Tally(ctx, n + 2)
    try:
        blobs = [v.g1_vector_to_blob(cref.saver_encrypt_ct(n, pk_w, gabc, fr_array(m), fr_array([o.rand_fr(gen)])[0])) for m in ballots]
        status, accepted = tally.add_blobs(blobs)
        assert accepted == 4 and not status.any()
        agg, _ = tally.result()
    finally:
        tally.free()
    with v.SaverDecryptor(ctx, vk_w, gabc, n, 1 << 20) as dec:
        assert dec.baby_bits == 11
        msgs, nu, status = v.saver_decrypt_batch(ctx, dec, sk, agg)
        assert msgs.tolist() == [[70002, 1]] and status.tolist() == [[0, 0]]
        vk, gabc_o, ct_o = sv.vk_from_words(vk_w, n), [o.g1_from_limbs(x) for x in gabc], [o.g1_from_limbs(x) for x in agg]
        nu_o = o.g1_from_limbs(nu[0])
        assert sv.verify_decryption(vk, gabc_o, ct_o, [70002, 1], nu_o)
        bad_nu = o.G1.add(nu_o, o.G1.gen)
        assert not sv.verify_decryption(vk, gabc_o, ct_o, [70002, 1], bad_nu)
        verdict, reason, first = v.saver_verify_decryption_batch(ctx, dec, np.stack([agg, agg, agg]), [[70002, 1], [70002, 1], [70002, 2]],
                                                                 np.stack([nu[0], g1_limbs(bad_nu), nu[0]]))
        assert verdict.tolist() == [1, 0, 0] and reason.tolist() == [0, 6, 4] and first.tolist() == [NO_SLOT, 0, 1]


def test_base_is_the_pairing_of_the_key_members(ctx):
    rg = make_rng(10)
    key = dd.DecryptKey(rg, 3)
    with decryptor(ctx, key, 10) as dec:
        W = key.vk_words.reshape(-1, 24)[1 + 3:]
        gt, _ = v.multi_pairing_batch(ctx, key.gamma_abc[1:], W, 1)
        for i in range(3):
            assert dec.base(i) == gt[i].tobytes()
        out = np.zeros(576, np.uint8)
        assert ctx.lib.vsp_saver_decryptor_base(dec.h, 3, v.api._ptr(out)) != 0 and ctx.lib.vsp_saver_decryptor_base(None, 0, v.api._ptr(out)) != 0


def test_refusals_leave_the_context_usable(ctx):
    rg = make_rng(11)
    key = dd.DecryptKey(rg, 2)
    lib, p = ctx.lib, v.api._ptr
    gabc, words = np.ascontiguousarray(key.gamma_abc), key.vk_words.copy()
    ERR_ARG = lib.vsp_saver_decrypt_batch(None, None, None, None, 0, None, None, None)
    assert ERR_ARG != 0
    # degenerate keys: W_1 at infinity, G_2 at infinity
    bad = words.copy(); bad[24 + 24 * 2:24 + 24 * 3] = 0
    assert not lib.vsp_saver_decryptor_create(ctx.h, 2, p(bad), p(gabc), 100) and "degenerate" in ctx.last_error()
    bad_g = gabc.copy(); bad_g[2] = 0
    with pytest.raises(v.VspError, match="degenerate"):
        v.SaverDecryptor(ctx, words, bad_g, 2, 100)
    off = words.copy(); off[24 + 13] ^= np.uint64(1)                                         # V_1 off its curve
    with pytest.raises(v.VspError, match="curve"):
        v.SaverDecryptor(ctx, off, gabc, 2, 100)
    # more than 2^24 giant steps at the forced baby bits; options outside their ranges
    try:
        ctx.set_option("saver_decrypt_baby_bits", 1)
        assert not lib.vsp_saver_decryptor_create(ctx.h, 2, p(words), p(gabc), 1 << 25) and "2^24" in ctx.last_error()
        ctx.set_option("saver_decrypt_baby_bits", 21)
        assert not lib.vsp_saver_decryptor_create(ctx.h, 2, p(words), p(gabc), 100)
        ctx.set_option("saver_decrypt_baby_bits", 0)
        ctx.set_option("saver_decrypt_fp_bits", 65)
        assert not lib.vsp_saver_decryptor_create(ctx.h, 2, p(words), p(gabc), 100)
    finally:
        ctx.set_option("saver_decrypt_baby_bits", 0)
        ctx.set_option("saver_decrypt_fp_bits", 64)
    assert not lib.vsp_saver_decryptor_create(ctx.h, 0, p(words), p(gabc), 100) and not lib.vsp_saver_decryptor_create(ctx.h, 2, None, p(gabc), 100)
    with decryptor(ctx, key, 100) as dec:
        us = key.ciphertext([4, 100], rg)
        ct = dd.ct_batch(key, [us])
        msgs, nu, st = np.zeros((1, 2), np.uint64), np.zeros((1, 12), np.uint64), np.zeros((1, 2), np.uint8)
        big = fr_array([R])[0]
        assert lib.vsp_saver_decrypt_batch(ctx.h, dec.h, p(big), p(ct), 1, p(msgs), p(nu), p(st)) == ERR_ARG and "rho" in ctx.last_error()
        assert lib.vsp_saver_decrypt_batch(ctx.h, dec.h, None, None, 0, None, None, None) == ERR_ARG          # also with count = 0
        assert lib.vsp_saver_decrypt_batch(ctx.h, None, p(key.rho_limbs), p(ct), 1, p(msgs), p(nu), p(st)) == ERR_ARG
        assert lib.vsp_saver_decrypt_batch(ctx.h, dec.h, p(key.rho_limbs), p(ct), 0, p(msgs), p(nu), p(st)) == 0  # nothing to do
        verdict = np.zeros(1, np.uint8)
        m4 = dd.scalars([[4, 100]])
        assert lib.vsp_saver_verify_decryption_batch(ctx.h, dec.h, None, None, None, 0, None, None, None) == ERR_ARG
        assert lib.vsp_saver_verify_decryption_batch(None, dec.h, p(ct), p(m4), p(nu), 1, p(verdict), None, None) == ERR_ARG
        assert lib.vsp_saver_verify_decryption_batch(ctx.h, dec.h, p(ct), p(m4), p(nu), 0, p(verdict), None, None) == 0
        # the context is usable afterwards, and the optional outputs may be null
        assert lib.vsp_saver_decrypt_batch(ctx.h, dec.h, p(key.rho_limbs), p(ct), 1, p(msgs), None, p(st)) == 0
        assert msgs.tolist() == [[4, 100]] and st.tolist() == [[0, 0]]
        _, nu, _ = v.saver_decrypt_batch(ctx, dec, key.rho_limbs, ct)
        assert lib.vsp_saver_verify_decryption_batch(ctx.h, dec.h, p(ct), p(m4), p(nu), 1, p(verdict), None, None) == 0 and verdict.tolist() == [1]
        assert lib.vsp_saver_decryptor_msg_size(None) == 0 and lib.vsp_saver_decryptor_max_value(None) == 0 and lib.vsp_saver_decryptor_baby_bits(None) == 0
