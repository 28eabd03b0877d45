"""GPU: vsp_saver_verify_batch -- verify_encryption verdicts for ballots made by vsp_saver_encrypt and vsp_saver_rerandomize: 66 ballots at
msg_size 4 across the 64-lane block edge, every piece and grouping, tampered and malformed members rejected one by one with their
reasons, four ballots cross-checked with oracle/saver.py verify_encryption, and two ballots at the real msg_size 25.

The election key is made with s_1 = s_2 and s_3 = r - s_1, and half of the ballots vote at position 4 (m_1 = m_2 = m_3 = 0): those
valid ballots have c_1 = c_2 = -c_3, so the accumulation of the ciphertext into the public-input point doubles and cancels."""
import ctypes as C

import numpy as np
import pytest

import bls12_381 as o
import saver as sv
from conftest import I, L, fr_array, g1_limbs

import vote_saver_protocol_amd as v

pytestmark = pytest.mark.gpu
N, NC, NI, K = 4, 48, 6, 66
VOTES = (0, 3, 1, 3, 2, 3)                                          # one real ballot each, rerandomized 11 times: 66


def _gg_vk(parts):
    return dict(alpha_g1=o.g1_from_limbs(parts["alpha_g1"][0]), beta_g2=o.g2_from_limbs(parts["beta_g2"][0]),
                gamma_g2=o.g2_from_limbs(parts["gamma_g2"][0]), delta_g2=o.g2_from_limbs(parts["delta_g2"][0]),
                gamma_ABC_g1=[o.g1_from_limbs(x) for x in parts["gamma_ABC_g1"]])


def _ct_points(ct):
    return [o.g1_from_limbs(row) for row in np.asarray(ct).reshape(-1, 12)]


def _setup(ctx, cref, n, nc, ni, seed, votes, copies, special_s):
    """an election: Groth16 key of a synthetic system whose first n public inputs are the one-hot ballot, SAVER key, and
    len(votes) * copies distinct ballots (each real ballot rerandomized `copies` times)"""
    gen = o.splitmix64(seed)
    tox = fr_array([o.rand_fr(gen) for _ in range(5)])
    rnd_i = [o.rand_fr(gen) for _ in range(3 * n + 2)]
    if special_s:
        rnd_i[1] = rnd_i[0]; rnd_i[2] = o.R - rnd_i[0]
    rnd = fr_array(rnd_i)
    dcs = kp = spk = parts = None
    cts, As, Bs, Cs, rests = [], [], [], [], []
    for vote in votes:
        cs, wit = cref.R1CS.synth(nc, ni, seed, ballot=(n, vote))    # the same system, another ballot
        assert [I(x) for x in wit[:n]] == [1 if i == vote else 0 for i in range(n)]
        if dcs is None:
            dcs = v.R1CS(ctx, nc, ni, cs.num_vars, *cs.export())
            kp = v.Keypair(ctx, dcs, tox)
            parts = {k: kp.part(k) for k in ("gamma_ABC_g1", "delta_g1", "gamma_g1", "alpha_g1", "beta_g2", "gamma_g2", "delta_g2")}
            gabc = np.ascontiguousarray(parts["gamma_ABC_g1"])
            pk_w, _, _ = v.saver_generate_keypair(ctx, rnd, gabc, parts["delta_g1"][0], parts["gamma_g1"][0], n)
            spk = v.SaverPublicKey(ctx, pk_w, gabc[:n + 1], n)
        r_enc, r, s = (L(o.rand_fr(gen), 4) for _ in range(3))
        ct, abc, _ = v.saver_encrypt(ctx, spk, dcs, kp.pk, wit[:n], wit, r_enc, r, s)
        for _ in range(copies):
            ct, abc, _ = v.saver_rerandomize(ctx, spk, parts["delta_g2"][0], fr_array([o.rand_fr(gen) for _ in range(3)]), ct, abc)
            cts.append(ct); As.append(abc[0].reshape(12)); Bs.append(abc[1].reshape(24)); Cs.append(abc[2].reshape(12)); rests.append(wit[n:ni].copy())
        cs.free()
    ver = v.SaverVerifier(ctx, pk_w, parts["alpha_g1"][0], parts["beta_g2"][0], parts["gamma_g2"][0], parts["delta_g2"][0], parts["gamma_ABC_g1"], n)
    e = dict(ver=ver, parts=parts, pk_w=pk_w, ct=np.stack(cts), rest=np.stack(rests), A=np.stack(As), B=np.stack(Bs), C=np.stack(Cs))
    return e, (ver, spk, kp, dcs)


@pytest.fixture(scope="module")
def election(ctx, cref):
    e, handles = _setup(ctx, cref, N, NC, NI, 404, VOTES, K // len(VOTES), special_s=True)
    assert e["ver"].msg_size == N and e["ct"].shape == (K, N + 2, 12) and e["rest"].shape == (K, NI - N, 4)
    assert len({c.tobytes() for c in e["ct"]}) == K
    for k in (11, 21, 33, 65):                                       # position 4: the doubling and cancelling members
        c = e["ct"][k]
        assert np.array_equal(c[1], c[2]) and np.array_equal(c[3], g1_limbs(o.G1.neg(o.g1_from_limbs(c[1])))) and c[1].any()
    yield e
    for h in handles:
        h.free()


def verify(ctx, e, ct=None, rest=None, A=None, B=None, Cc=None, sl=slice(None)):
    pick = lambda x, d: (d if x is None else x)[sl]
    verdict, reason = v.saver_verify_batch(ctx, e["ver"], pick(ct, e["ct"]), pick(rest, e["rest"]), pick(A, e["A"]), pick(B, e["B"]), pick(Cc, e["C"]))
    assert verdict.tolist() == [int(r == 0) for r in reason]
    return reason.tolist()


def oracle_verdict(e, n, ct, rest, A, B, Cc):
    return sv.verify_encryption(sv.pk_from_words(e["pk_w"], n), _gg_vk(e["parts"]), _ct_points(ct), (o.g1_from_limbs(A), o.g2_from_limbs(B), o.g1_from_limbs(Cc)),
                                [I(x) for x in rest])


def tampered(e):
    ct, rest, A, Cc = e["ct"].copy(), e["rest"].copy(), e["A"].copy(), e["C"].copy()
    ct[0, [1, 4]] = ct[0, [4, 1]]                                                  # c_1 and c_4 swapped: their sum is unchanged
    Cc[31] = g1_limbs(o.G1.neg(o.g1_from_limbs(Cc[31])))                           # C negated
    ct[32, N + 1] = g1_limbs(o.G1.neg(o.g1_from_limbs(ct[32, N + 1])))             # psi negated
    rest[63, 1] = L((I(rest[63, 1]) + 1) % o.R, 4)                                 # one rest input incremented
    ct[64, 0] = g1_limbs(o.G1.mul(o.g1_from_limbs(ct[64, 0]), 2))                  # c_0 replaced by 2 c_0
    A[65] = 0                                                                      # A = infinity
    return ct, rest, A, Cc


def test_every_ballot_is_accepted_in_every_piece_and_grouping(ctx, election):
    e = election
    assert verify(ctx, e) == [0] * K
    assert verify(ctx, e, sl=slice(12, 13)) == [0]                                 # n = 1
    ct, rest, A, Cc = tampered(e)
    want = verify(ctx, e, ct=ct, rest=rest, A=A, Cc=Cc)
    try:
        ctx.set_option("pairing_chunk", 20)
        assert verify(ctx, e) == [0] * K
        assert verify(ctx, e, ct=ct, rest=rest, A=A, Cc=Cc) == want
        ctx.set_option("pairing_chunk", 1 << 14)
        for group in (1, 2, 4):                                                    # groups of 1 x 6, 2 2 2, 4 2
            ctx.set_option("saver_verify_group", group)
            assert verify(ctx, e) == [0] * K, group
            assert verify(ctx, e, ct=ct, rest=rest, A=A, Cc=Cc) == want, group
    finally:
        ctx.set_option("pairing_chunk", 1 << 14)
        ctx.set_option("saver_verify_group", 9)


def test_tampered_ballots_are_rejected_with_their_reasons_and_only_they(ctx, election):
    e = election
    assert not np.array_equal(e["ct"][0, 1], e["ct"][0, 4])
    ct, rest, A, Cc = tampered(e)
    reason = verify(ctx, e, ct=ct, rest=rest, A=A, Cc=Cc)
    want = {0: 2, 31: 4, 32: 2, 63: 4, 64: 6, 65: 4}
    assert reason == [want.get(k, 0) for k in range(K)]


def test_malformed_ballots_get_reason_one_alone(ctx, election):
    e = election
    ct, rest, A = e["ct"].copy(), e["rest"].copy(), e["A"].copy()
    ct[7, 2, 6] ^= np.uint64(1)                                                    # a ciphertext point off the curve
    A[20, :6] = L(o.P, 6)                                                          # a coordinate equal to p
    rest[40, 1] = L(I(rest[40, 1]) + o.R, 4)                                       # the same scalar, not reduced
    assert verify(ctx, e, ct=ct, rest=rest, A=A) == [1 if k in (7, 20, 40) else 0 for k in range(K)]
    assert verify(ctx, e) == [0] * K


def test_four_ballots_agree_with_the_oracle(ctx, election):
    """an accepted ballot, a doubling and cancelling one, the swapped one, and one with an infinity ciphertext member (c_2 zeroed), for
    which the library's verdict must be the oracle's whatever it is"""
    e = election
    ct = np.stack([e["ct"][5], e["ct"][12], e["ct"][0], e["ct"][40]])
    ct[2, [1, 4]] = ct[2, [4, 1]]
    ct[3, 2] = 0
    idx = [5, 12, 0, 40]
    pick = lambda x: np.stack([x[k] for k in idx])
    verdict, reason = v.saver_verify_batch(ctx, e["ver"], ct, pick(e["rest"]), pick(e["A"]), pick(e["B"]), pick(e["C"]))
    want = [oracle_verdict(e, N, ct[i], e["rest"][k], e["A"][k], e["B"][k], e["C"][k]) for i, k in enumerate(idx)]
    assert want[:3] == [True, True, False]
    assert verdict.tolist() == [int(w) for w in want]
    assert reason.tolist()[:3] == [0, 0, 2] and reason[3] != 1


def test_real_shape_msg_size_25_default_grouping(ctx, cref):
    """two ballots at the reference's msg_size 25 (27 pairs in three groups of 9), the second with C negated; the first judged by the oracle too"""
    n, nc, ni = 25, 100, 30
    e, handles = _setup(ctx, cref, n, nc, ni, 2525, (7,), 2, special_s=False)
    try:
        Cc = e["C"].copy()
        Cc[1] = g1_limbs(o.G1.neg(o.g1_from_limbs(Cc[1])))
        verdict, reason = v.saver_verify_batch(ctx, e["ver"], e["ct"], e["rest"], e["A"], e["B"], Cc)
        assert verdict.tolist() == [1, 0] and reason.tolist() == [0, 4]
        assert oracle_verdict(e, n, e["ct"][0], e["rest"][0], e["A"][0], e["B"][0], e["C"][0])
    finally:
        for h in handles:
            h.free()


def test_errors_leave_the_context_usable(ctx, election):
    e = election
    lib, p = ctx.lib, v.api._ptr
    one = slice(3, 4)
    ct, rest, A, B, Cc = (np.ascontiguousarray(e[k][one]) for k in ("ct", "rest", "A", "B", "C"))
    verdict = np.zeros(1, np.uint8)
    ERR_ARG = lib.vsp_saver_verify_batch(None, e["ver"].h, p(ct), p(rest), p(A), p(B), p(Cc), 1, p(verdict), None)
    assert ERR_ARG != 0
    assert lib.vsp_saver_verify_batch(ctx.h, e["ver"].h, None, p(rest), p(A), p(B), p(Cc), 1, p(verdict), None) == ERR_ARG
    assert lib.vsp_saver_verify_batch(ctx.h, e["ver"].h, None, None, None, None, None, 0, None, None) == ERR_ARG       # also with n = 0
    assert lib.vsp_saver_verify_batch(ctx.h, None, p(ct), p(rest), p(A), p(B), p(Cc), 1, p(verdict), None) == ERR_ARG
    assert lib.vsp_saver_verify_batch(ctx.h, e["ver"].h, p(ct), p(rest), p(A), p(B), p(Cc), 0, p(verdict), None) == 0    # no ballots: nothing to do
    parts = e["parts"]
    args = lambda pk_w, gamma: (ctx, pk_w, parts["alpha_g1"][0], parts["beta_g2"][0], gamma, parts["delta_g2"][0], parts["gamma_ABC_g1"], N)
    bad_pk = e["pk_w"].copy(); bad_pk[12 + 24 * N + 24 + 12] ^= np.uint64(1)          # t_g2[1] off the curve
    with pytest.raises(v.VspError, match="curve"):
        v.SaverVerifier(*args(bad_pk, parts["gamma_g2"][0]))
    bad_gamma = parts["gamma_g2"][0].copy(); bad_gamma[13] ^= np.uint64(1)
    with pytest.raises(v.VspError, match="curve"):
        v.SaverVerifier(*args(e["pk_w"], bad_gamma))
    with pytest.raises(ValueError):
        v.SaverVerifier(ctx, e["pk_w"][:-1], *args(e["pk_w"], parts["gamma_g2"][0])[2:])
    assert lib.vsp_saver_verifier_msg_size(e["ver"].h) == N and lib.vsp_saver_verifier_msg_size(None) == 0
    assert verify(ctx, e, sl=one) == [0]
