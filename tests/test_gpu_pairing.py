"""GPU: vsp_multi_pairing_batch and the verification-key handle against the oracle's pairing.  Expected values come from ONE oracle
e(G1, G2) and f12_pow of it (bilinearity: e(a G1, b G2) = e(G1, G2)^(a b)), at most 16 distinct oracle values per test."""
import numpy as np
import pytest

import bls12_381 as o
import pairing as pg
import wire
from conftest import L, g1_limbs, g2_limbs

import vote_saver_protocol_amd as v

pytestmark = pytest.mark.gpu
ONE = wire.gt_to_tower_le(pg.ONE)
AB = [(1, 1), (2, 3), (5, 7), (o.R - 1, 1), (11, o.R - 2), (123456789, 987654321), (3, 1 << 200), ((1 << 254) % o.R, 9)]


@pytest.fixture(scope="module")
def e_gen():
    return pg.final_exp(pg.miller_loop(o.G2.gen, o.G1.gen))


@pytest.fixture(scope="module")
def pairs(e_gen):
    """8 distinct (a G1 limbs, b G2 limbs, 576 expected bytes)"""
    return [(g1_limbs(o.G1.mul(o.G1.gen, a)), g2_limbs(o.G2.mul(o.G2.gen, b)), wire.gt_to_tower_le(pg.f12_pow(e_gen, a * b % o.R))) for a, b in AB]


def shuffled(pairs, n, seed):
    idx = np.random.default_rng(seed).integers(0, len(pairs), size=n)
    return np.stack([pairs[i][0] for i in idx]), np.stack([pairs[i][1] for i in idx]), [pairs[i][2] for i in idx]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_batch_of_pairings_equals_the_oracle(ctx, pairs, n):
    g1, g2, want = shuffled(pairs, n, n)
    gt, is_one = v.multi_pairing_batch(ctx, g1, g2, 1)
    for k in range(n):
        assert gt[k].tobytes() == want[k], k
    assert not is_one.any()
    assert ctx.stat("pairing_miller_ms") > 0 and ctx.stat("pairing_finalexp_ms") > 0


def test_pieces_give_the_same_bytes(ctx, pairs):
    g1, g2, want = shuffled(pairs, 130, 7)
    whole = v.pairing_batch(ctx, g1, g2)
    ctx.set_option("pairing_chunk", 64)
    try:
        pieces = v.pairing_batch(ctx, g1, g2)
    finally:
        ctx.set_option("pairing_chunk", 1 << 14)
    assert np.array_equal(whole, pieces)
    assert [x.tobytes() for x in pieces] == want


def test_products(ctx, pairs, e_gen):
    n = 5
    neg = lambda p: g1_limbs(o.G1.neg(o.g1_from_limbs(p)))
    # m = 2: (P, Q), (-P, Q)
    g1 = np.stack([x for k in range(n) for x in (pairs[k][0], neg(pairs[k][0]))]); g2 = np.stack([x for k in range(n) for x in (pairs[k][1], pairs[k][1])])
    gt, is_one = v.multi_pairing_batch(ctx, g1, g2, 2)
    assert is_one.tolist() == [1] * n and all(x.tobytes() == ONE for x in gt)
    # m = 3, nothing cancels: exponents add
    tri = [(k, (k + 1) % 8, (k + 3) % 8) for k in range(n)]
    g1 = np.stack([pairs[i][0] for t in tri for i in t]); g2 = np.stack([pairs[i][1] for t in tri for i in t])
    gt, is_one = v.multi_pairing_batch(ctx, g1, g2, 3)
    for k, t in enumerate(tri):
        e = sum(AB[i][0] * AB[i][1] for i in t) % o.R
        assert gt[k].tobytes() == wire.gt_to_tower_le(pg.f12_pow(e_gen, e)), k
    assert not is_one.any()
    # the middle pair has infinity (on the G1 side in even products, on the G2 side in odd ones)
    for k in range(n):
        if k % 2 == 0:
            g1[3 * k + 1] = 0
        else:
            g2[3 * k + 1] = 0
    gt, is_one = v.multi_pairing_batch(ctx, g1, g2, 3)
    for k, t in enumerate(tri):
        e = (AB[t[0]][0] * AB[t[0]][1] + AB[t[2]][0] * AB[t[2]][1]) % o.R
        assert gt[k].tobytes() == wire.gt_to_tower_le(pg.f12_pow(e_gen, e)), k
    # infinity alone is one
    gt, is_one = v.multi_pairing_batch(ctx, np.zeros((1, 12), np.uint64), pairs[0][1].reshape(1, 24), 1)
    assert is_one.tolist() == [1] and gt[0].tobytes() == ONE


def test_error_paths(ctx, pairs):
    g1, g2, want = shuffled(pairs, 70, 3)
    ok = lambda: [x.tobytes() for x in v.pairing_batch(ctx, g1, g2)] == want
    bad1 = g1.copy(); bad1[66, 6] ^= np.uint64(1)                     # y of a G1 point: off the curve
    bad2 = g2.copy(); bad2[3, 0] ^= np.uint64(1)                      # x.c0 of a G2 point
    badp = g1.copy(); badp[69, :6] = L(o.P, 6)                        # a coordinate equal to p
    lib = ctx.lib
    out = np.zeros((70, 576), np.uint8); one = np.zeros(70, np.uint8)
    p = v.api._ptr
    for a, b in ((bad1, g2), (g1, bad2), (badp, g2)):
        assert lib.vsp_multi_pairing_batch(ctx.h, p(a), p(b), 1, 70, p(out), p(one)) == -1          # VSP_ERR_ARG
        with pytest.raises(v.VspError, match="vsp error -1"):
            v.pairing_batch(ctx, a, b)
        assert ok()
    assert lib.vsp_multi_pairing_batch(ctx.h, p(g1), p(g2), (1 << 16) + 1, 0, p(out), p(one)) == -1     # m above 2^16
    assert lib.vsp_multi_pairing_batch(ctx.h, None, p(g2), 1, 70, p(out), p(one)) == -1
    assert lib.vsp_multi_pairing_batch(ctx.h, p(g1), None, 1, 0, p(out), p(one)) == -1
    assert lib.vsp_multi_pairing_batch(ctx.h, p(g1), p(g2), 0, 70, p(out), p(one)) == -1
    assert lib.vsp_multi_pairing_batch(None, p(g1), p(g2), 1, 70, p(out), p(one)) == -1
    assert lib.vsp_multi_pairing_batch(ctx.h, p(g1), p(g2), 1, 70, None, p(one)) == 0 and not one.any()      # gt_out = NULL
    assert ok()


def test_vk_alpha_beta_and_blob_round_trip(ctx, pairs, e_gen):
    a, b = 5, 7
    alpha, beta = pairs[2][0], pairs[2][1]
    gamma, delta = g2_limbs(o.G2.mul(o.G2.gen, 13)), g2_limbs(o.G2.mul(o.G2.gen, 17))
    gabc = np.stack([pairs[k][0] for k in range(4)])
    vk = v.VerifyingKey(ctx, alpha, beta, gamma, delta, gabc)
    gt = vk.alpha_beta()
    assert gt == wire.gt_to_tower_le(pg.f12_pow(e_gen, a * b))
    blob = v.vk_to_blob(gt, gamma, delta, pairs[1][0], gabc, pairs[3][0])
    back = v.vk_from_blob(blob)
    assert back["alpha_g1_beta_g2"] == gt and np.array_equal(back["gamma_g2"], gamma) and np.array_equal(back["gamma_ABC_g1"], gabc)
    vk.free()
    bad = alpha.copy(); bad[6] ^= np.uint64(1)
    with pytest.raises(v.VspError):
        v.VerifyingKey(ctx, bad, beta, gamma, delta, gabc)
