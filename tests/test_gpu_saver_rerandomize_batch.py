"""GPU: vsp_saver_rerandomize_batch -- the ballot box's rerandomization of many ballots a call, over the key's device tables and the
rerandomizer's table of delta_g2.

Every member is checked against vsp_saver_rerandomize on the same inputs and against the C oracle's saver_rerandomize, in limbs, proof
bytes and blobs, some against oracle/saver.py rerandomize.  The inputs are curve points, not valid ballots (multiples of the generators
through the oracle), but in the last test, where real ballots of vsp_saver_encrypt_batch go through rerandomization, both verifiers and
the tally."""
import ctypes as C

import numpy as np
import pytest

import bls12_381 as o
import saver as sv
from conftest import I, L, fr_array, g1_limbs, g2_limbs
from test_gpu_saver_encrypt_batch import saver_key
from test_gpu_saver_verify import N, NC, NI, _setup

import vote_saver_protocol_amd as v

pytestmark = pytest.mark.gpu
ERR_ARG = "vsp error -1"
M = 67                                                              # members: more than one workgroup of every kernel, the last one not full


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def scalars_of(count, seed):
    """rnd [count, 3, 4]: r' 0, 1, R - 1, random by member; z1 1, R - 1, random every four members; z2 0, 1, R - 1, random every twelve"""
    gen = o.splitmix64(seed)
    rows = []
    for k in range(count):
        rows += [(0, 1, o.R - 1, o.rand_fr(gen))[k % 4], (1, o.R - 1, o.rand_fr(gen))[(k // 4) % 3], (0, 1, o.R - 1, o.rand_fr(gen))[(k // 12) % 4]]
    return fr_array(rows).reshape(count, 3, 4)


def points_of(cref, n, count, seed):
    """ct [count, n + 2, 12], A, B, C: multiples of the generators"""
    gen = o.splitmix64(seed)
    g1 = cref.g1_batch_mul_gen(fr_array([o.rand_fr(gen) for _ in range(count * (n + 4))])).reshape(count, n + 4, 12)
    B = cref.g2_batch_mul_gen(fr_array([o.rand_fr(gen) for _ in range(count)]))
    return np.ascontiguousarray(g1[:, :n + 2]), np.ascontiguousarray(g1[:, n + 2]), np.ascontiguousarray(B), np.ascontiguousarray(g1[:, n + 3])


def proof_bytes(A, B, Cc):
    return v.g1_compress(A) + v.g2_compress(B) + v.g1_compress(Cc)


def oracle_member(cref, e, rnd, ct, A, B, Cc):
    ct2, A2, B2, C2 = cref.saver_rerandomize(e["n"], e["pk_w"], e["delta_g2"], rnd.reshape(12), ct, A, B, Cc)
    return ct2, A2, B2, C2


@pytest.fixture(scope="module")
def plain(ctx, cref):
    """per msg_size: the key, delta_g2, the rerandomizer, M members and the C oracle's outputs of each, computed once"""
    out = {}
    for n in (3, 25):
        pk_w, _, _, gabc = saver_key(ctx, cref, n, 800 + n)
        delta_g2 = cref.g2_batch_mul_gen(fr_array([o.rand_fr(o.splitmix64(810 + n))]))[0]
        spk = v.SaverPublicKey(ctx, pk_w, gabc, n)
        rr = v.SaverRerandomizer(ctx, spk, delta_g2)
        e = dict(n=n, pk_w=pk_w, delta_g2=delta_g2, spk=spk, rr=rr, rnd=scalars_of(M, 820 + n))
        e["ct"], e["A"], e["B"], e["C"] = points_of(cref, n, M, 830 + n)
        e["want"] = [oracle_member(cref, e, e["rnd"][k], e["ct"][k], e["A"][k], e["B"][k], e["C"][k]) for k in range(M)]
        out[n] = e
    yield out
    for e in out.values():
        e["rr"].free(); e["spk"].free()


def batch(ctx, e, sl=slice(None), **kw):
    return v.saver_rerandomize_batch(ctx, e["rr"], e["rnd"][sl], e["ct"][sl], (e["A"][sl], e["B"][sl], e["C"][sl]), **kw)


def check_member(got, j, want, tag):
    ct, (A, B, Cc), proofs, blobs, st = got
    assert st[j] == 0, tag
    assert np.array_equal(ct[j], want[0]), tag
    assert np.array_equal(A[j], want[1]) and np.array_equal(B[j], want[2]) and np.array_equal(Cc[j], want[3]), tag
    assert proofs[j] == proof_bytes(want[1], want[2], want[3]) and blobs[j] == v.g1_vector_to_blob(want[0]), tag


@pytest.mark.parametrize("n", [3, 25])
def test_members_equal_the_single_call_and_the_oracles(ctx, plain, n):
    e = plain[n]
    assert e["rr"].device_bytes >= 960 * 192 and e["spk"].device_bytes >= (3 * n + 3) * 92160
    assert ctx.lib.vsp_saver_rerandomizer_msg_size(e["rr"].h) == n and ctx.lib.vsp_saver_rerandomizer_msg_size(None) == 0
    before = ctx.stat("saver_rerandomize_ballots")
    for count in (1, 2, M):
        got = batch(ctx, e, slice(0, count))
        for k in range(count):
            check_member(got, k, e["want"][k], (count, k))
    assert ctx.stat("saver_rerandomize_ballots") == before + 1 + 2 + M and ctx.stat("saver_rerandomize_ms") > 0
    for k in range(M):                                              # the single call, byte for byte
        ct, (A, B, Cc), proof = v.saver_rerandomize(ctx, e["spk"], e["delta_g2"], e["rnd"][k], e["ct"][k], (e["A"][k], e["B"][k], e["C"][k]))
        assert np.array_equal(ct, got[0][k]) and proof == got[2][k], k
        assert np.array_equal(A, got[1][0][k]) and np.array_equal(B, got[1][1][k]) and np.array_equal(Cc, got[1][2][k]), k
    pk_o, d2 = sv.pk_from_words(e["pk_w"], n), o.g2_from_limbs(e["delta_g2"])
    for k in (3, 21, 50):                                           # random r' under z1 = 1; 1, R - 1, 1; R - 1, 1, 0
        ct2, (A2, B2, C2) = sv.rerandomize(pk_o, d2, [I(x) for x in e["rnd"][k]], [o.g1_from_limbs(x) for x in e["ct"][k]],
                                           (o.g1_from_limbs(e["A"][k]), o.g2_from_limbs(e["B"][k]), o.g1_from_limbs(e["C"][k])))
        assert np.array_equal(got[0][k], np.stack([g1_limbs(p) for p in ct2])), k
        assert np.array_equal(got[1][0][k], g1_limbs(A2)) and np.array_equal(got[1][1][k], g2_limbs(B2)) and np.array_equal(got[1][2][k], g1_limbs(C2)), k


def same(a, b):
    return (np.array_equal(a[0], b[0]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1])) and a[2] == b[2] and a[3] == b[3] and np.array_equal(a[4], b[4]))


def join(a, b):
    return (np.concatenate([a[0], b[0]]), tuple(np.concatenate([x, y]) for x, y in zip(a[1], b[1])), a[2] + b[2], a[3] + b[3], np.concatenate([a[4], b[4]]))


@pytest.mark.parametrize("n", [3, 25])
def test_pieces_calls_and_outputs_over_the_inputs_give_the_same_bytes(ctx, plain, n):
    e = plain[n]
    whole = batch(ctx, e)
    check_member(whole, M - 1, e["want"][M - 1], "whole")
    assert same(join(batch(ctx, e, slice(0, 30)), batch(ctx, e, slice(30, M))), whole)
    for option, value, back in (("saver_rerandomize_chunk", 16, 1 << 16), ("saver_rerandomize_w4", 0, 1)):
        ctx.set_option(option, value)
        try:
            assert same(batch(ctx, e), whole), option
        finally:
            ctx.set_option(option, back)
    ct, A, B, Cc = e["ct"].copy(), e["A"].copy(), e["B"].copy(), e["C"].copy()
    got = v.saver_rerandomize_batch(ctx, e["rr"], e["rnd"], ct, (A, B, Cc), in_place=True)
    assert same(got, whole) and np.array_equal(ct, whole[0]) and np.array_equal(A, whole[1][0]) and np.array_equal(B, whole[1][1]) and np.array_equal(Cc, whole[1][2])
    # some outputs only
    ct2, abc, proofs, blobs, st = batch(ctx, e, slice(0, 5), proofs=False, blobs=False)
    assert proofs is None and blobs is None and np.array_equal(ct2, whole[0][:5]) and not st.any()
    pr = np.zeros((5, 192), np.uint8)
    rc = ctx.lib.vsp_saver_rerandomize_batch(ctx.h, e["rr"].h, _p(e["rnd"]), _p(e["ct"]), _p(e["A"]), _p(e["B"]), _p(e["C"]), 5, None, None, None, None, _p(pr), None, None)
    assert rc == 0 and [pr[k].tobytes() for k in range(5)] == whole[2][:5]


def test_exceptional_sums(ctx, cref):
    """msg_size 3; oracle/saver.py computes what is expected.  0: ct_0 = r' X_0, the addition doubles.  1: ct_1 = -r' X_1 gives infinity.
    2: ct_2 at infinity.  3: A at infinity.  4: B at infinity, B' = z2 delta_g2.  5: B = -(z1 z2) delta_g2, B' at infinity.
    6: C = -((z1 z2) A + r' P2), C' at infinity.  7: all of them at once.  Then a key with X_1 at infinity: its table is flagged"""
    n = 3
    pk_w, _, _, gabc = saver_key(ctx, cref, n, 901)
    gen = o.splitmix64(902)
    d2 = o.G2.mul(o.G2.gen, o.rand_fr(gen))
    delta_g2 = g2_limbs(d2)
    pk_o = sv.pk_from_words(pk_w, n)
    X = [pk_o["delta_g1"]] + pk_o["delta_s_g1"] + [pk_o["delta_sum_s_g1"]]
    P2 = pk_o["gamma_inverse_sum_s_g1"]
    ct, A, B, Cc = points_of(cref, n, 8, 903)
    rnd = fr_array([o.rand_fr(gen) for _ in range(24)]).reshape(8, 3, 4)
    rnd[0, 0] = L(1 << 252, 4)                                       # one digit: lane 0 meets the given point with a single table entry
    for k in range(8):
        rp, z1, z2 = (I(x) for x in rnd[k])
        all_ = k == 7
        if k == 0 or all_:
            ct[k, 0] = g1_limbs(o.G1.mul(X[0], rp))
        if k == 1 or all_:
            ct[k, 1] = g1_limbs(o.G1.neg(o.G1.mul(X[1], rp)))
        if k == 2 or all_:
            ct[k, 2] = 0
        if k == 3:
            A[k] = 0
        if k == 4:
            B[k] = 0
        if k == 5 or all_:
            B[k] = g2_limbs(o.G2.neg(o.G2.mul(d2, z1 * z2 % o.R)))
        if k == 6 or all_:
            Cc[k] = g1_limbs(o.G1.neg(o.G1.add(o.G1.mul(o.g1_from_limbs(A[k]), z1 * z2 % o.R), o.G1.mul(P2, rp))))
    spk = v.SaverPublicKey(ctx, pk_w, gabc, n)
    rr = v.SaverRerandomizer(ctx, spk, delta_g2)
    try:
        got = v.saver_rerandomize_batch(ctx, rr, rnd, ct, (A, B, Cc))
        for k in range(8):
            ct2, (A2, B2, C2) = sv.rerandomize(pk_o, d2, [I(x) for x in rnd[k]], [o.g1_from_limbs(x) for x in ct[k]],
                                               (o.g1_from_limbs(A[k]), o.g2_from_limbs(B[k]), o.g1_from_limbs(Cc[k])))
            check_member(got, k, (np.stack([g1_limbs(p) for p in ct2]), g1_limbs(A2), g2_limbs(B2), g1_limbs(C2)), k)
        g_ct, (g_A, g_B, g_C), proofs, blobs, _ = got
        assert np.array_equal(g_ct[0, 0], g1_limbs(o.G1.mul(X[0], 2 * I(rnd[0, 0]) % o.R)))
        assert not g_ct[1, 1].any() and blobs[1][8 + 48:8 + 96] == o.g1_compress(None)
        assert np.array_equal(g_ct[2, 2], g1_limbs(o.G1.mul(X[2], I(rnd[2, 0]))))
        assert not g_A[3].any() and np.array_equal(g_B[4], g2_limbs(o.G2.mul(d2, I(rnd[4, 2]))))
        assert not g_B[5].any() and not g_C[6].any() and proofs[6][144:] == o.g1_compress(None)
        assert not g_ct[7, 1].any() and not g_B[7].any() and not g_C[7].any()
    finally:
        rr.free(); spk.free()
    # X_1 = delta_s_g1[0] at infinity, and delta_g2 at infinity
    flagged = pk_w.copy(); flagged[12:24] = 0
    spk = v.SaverPublicKey(ctx, flagged, gabc, n)
    rr = v.SaverRerandomizer(ctx, spk, np.zeros(24, np.uint64))
    try:
        got = v.saver_rerandomize_batch(ctx, rr, rnd[:3], ct[:3], (A[:3], B[:3], Cc[:3]))
        for k in range(3):
            want = cref.saver_rerandomize(n, flagged, np.zeros(24, np.uint64), rnd[k].reshape(12), ct[k], A[k], B[k], Cc[k])
            check_member(got, k, want, ("flagged", k))
            single = v.saver_rerandomize(ctx, spk, np.zeros(24, np.uint64), rnd[k], ct[k], (A[k], B[k], Cc[k]))
            assert np.array_equal(single[0], got[0][k]) and single[2] == got[2][k]
            assert np.array_equal(got[0][k, 1], ct[k, 1])
            assert np.array_equal(got[1][1][k], cref.g2_mul(B[k], L(pow(I(rnd[k, 1]), -1, o.R), 4)))
    finally:
        rr.free(); spk.free()


def test_refusals_before_any_gpu_work_name_the_member(ctx, plain):
    e = plain[3]
    before = ctx.stat("saver_rerandomize_ballots")
    for member, slot, value, text in ((5, 0, o.R, "r' of member 5"), (66, 2, o.R, "z2 of member 66"), (0, 1, o.R + 1, "z1 of member 0"), (1, 1, 0, "z1 of member 1 must be invertible")):
        rnd = e["rnd"].copy(); rnd[member, slot] = L(value, 4)
        with pytest.raises(v.VspError, match=ERR_ARG + ".*" + text):
            v.saver_rerandomize_batch(ctx, e["rr"], rnd, e["ct"], (e["A"], e["B"], e["C"]))
    args = [_p(e[k]) for k in ("rnd", "ct", "A", "B", "C")]
    out = np.zeros((M, 5, 12), np.uint64)
    for i in range(5):
        a = list(args); a[i] = None
        assert ctx.lib.vsp_saver_rerandomize_batch(ctx.h, e["rr"].h, *a, M, _p(out), None, None, None, None, None, None) == -1 and "null" in ctx.last_error(), i
    assert ctx.lib.vsp_saver_rerandomize_batch(ctx.h, None, *args, M, _p(out), None, None, None, None, None, None) == -1
    assert ctx.lib.vsp_saver_rerandomize_batch(None, e["rr"].h, *args, M, _p(out), None, None, None, None, None, None) == -1
    assert ctx.lib.vsp_saver_rerandomize_batch(ctx.h, e["rr"].h, None, None, None, None, None, 0, None, None, None, None, None, None, None) == 0      # no ballots: nothing to do
    assert ctx.stat("saver_rerandomize_ballots") == before and not out.any()
    bad = e["delta_g2"].copy(); bad[13] ^= np.uint64(1)
    with pytest.raises(v.VspError, match="curve"):
        v.SaverRerandomizer(ctx, e["spk"], bad)
    bad = e["delta_g2"].copy(); bad[:6] = L(o.P, 6)
    with pytest.raises(v.VspError, match="curve"):
        v.SaverRerandomizer(ctx, e["spk"], bad)
    check_member(batch(ctx, e, slice(0, 2)), 1, e["want"][1], "after the refusals")


@pytest.mark.parametrize("kind", ["ct off the curve", "psi off the curve", "A off the curve", "B off the curve", "C off the curve", "a coordinate of ct equal to p",
                                  "a coordinate of B above p"])
def test_a_bad_point_zeroes_its_member_alone(ctx, plain, kind):
    """at the first, a middle and the last member"""
    e = plain[3]
    n = 3
    ct, A, B, Cc = e["ct"].copy(), e["A"].copy(), e["B"].copy(), e["C"].copy()
    where = (0, 33, M - 1)
    for k in where:
        if kind == "ct off the curve":
            ct[k, 1, 6] ^= np.uint64(1)
        elif kind == "psi off the curve":
            ct[k, n + 1, 0] ^= np.uint64(2)
        elif kind == "A off the curve":
            A[k, 7] ^= np.uint64(1)
        elif kind == "B off the curve":
            B[k, 18] ^= np.uint64(1)
        elif kind == "C off the curve":
            Cc[k, 0] ^= np.uint64(1)
        elif kind == "a coordinate of ct equal to p":
            ct[k, 0, :6] = L(o.P, 6)
        else:
            B[k, 6:12] = L(o.P + 5, 6)
    got = v.saver_rerandomize_batch(ctx, e["rr"], e["rnd"], ct, (A, B, Cc))
    g_ct, (g_A, g_B, g_C), proofs, blobs, st = got
    assert st.tolist() == [int(k in where) for k in range(M)]
    for k in range(M):
        if k in where:
            assert not g_ct[k].any() and not g_A[k].any() and not g_B[k].any() and not g_C[k].any()
            assert proofs[k] == bytes(192) and blobs[k] == bytes(len(blobs[k]))
        else:
            check_member(got, k, e["want"][k], (kind, k))
    with pytest.raises(v.VspError, match=ERR_ARG + ".*member 0 is not a curve point"):
        v.saver_rerandomize_batch(ctx, e["rr"], e["rnd"], ct, (A, B, Cc), status=False)
    with pytest.raises(v.VspError, match=ERR_ARG + ".*member 32 "):
        v.saver_rerandomize_batch(ctx, e["rr"], e["rnd"][1:], ct[1:], (A[1:], B[1:], Cc[1:]), status=False)


def test_real_ballots_verify_tally_and_stay_invalid_when_they_were(ctx, cref):
    """the small system of test_gpu_saver_verify.py: a dozen ballots of vsp_saver_encrypt_batch rerandomized in one call pass both
    verifiers, their tally decrypts to the votes; a ballot whose C was negated before still fails with the same reason; and while a batch
    of proofs is in flight the call is refused"""
    seed = 909
    e, handles = _setup(ctx, cref, N, NC, NI, seed, (0,), 1, special_s=True)
    ver, spk, kp, dcs = handles
    parts = e["parts"]
    # the election's secret and verification keys: the random values _setup drew
    gen = o.splitmix64(seed)
    [o.rand_fr(gen) for _ in range(5)]
    rnd_i = [o.rand_fr(gen) for _ in range(3 * N + 2)]
    rnd_i[1] = rnd_i[0]; rnd_i[2] = o.R - rnd_i[0]
    gabc = np.ascontiguousarray(parts["gamma_ABC_g1"])
    pk_w, sk, vk_w = v.saver_generate_keypair(ctx, fr_array(rnd_i), gabc, parts["delta_g1"][0], parts["gamma_g1"][0], N)
    assert np.array_equal(pk_w, e["pk_w"])
    votes = [0, 3, 1, 3, 2, 3, 0, 1, 2, 3, 3, 1]
    W = []
    for vote in votes:
        cs, wit = cref.R1CS.synth(NC, NI, seed, ballot=(N, vote))
        W.append(wit); cs.free()
    W = np.stack(W)
    gen = o.splitmix64(seed + 1)
    rand = lambda k: fr_array([o.rand_fr(gen) for _ in range(k)])
    rr = v.SaverRerandomizer(ctx, spk, parts["delta_g2"][0])
    tally = v.Tally(ctx, N + 2)
    try:
        ct, (A, B, Cc), _, _ = v.saver_encrypt_batch(ctx, spk, dcs, kp.pk, np.ascontiguousarray(W[:, :N]), W, rand(12), rand(12), rand(12))
        rest = np.ascontiguousarray(W[:, N:NI])
        rnd = rand(36).reshape(12, 3, 4)
        ct2, abc2, proofs, blobs, st = v.saver_rerandomize_batch(ctx, rr, rnd, ct, (A, B, Cc))
        assert not st.any() and len({c.tobytes() for c in ct2} | {c.tobytes() for c in ct}) == 24
        for check in (v.saver_verify_batch, v.saver_verify_batch_screened):
            verdict, reason = check(ctx, ver, ct2, rest, *abc2)
            assert verdict.tolist() == [1] * 12 and not reason.any(), check.__name__
        assert proofs[4] == v.g1_compress(abc2[0][4]) + v.g2_compress(abc2[1][4]) + v.g1_compress(abc2[2][4])
        status, accepted = tally.add_blobs(blobs)
        assert accepted == 12 and not status.any()
        agg, _ = tally.result()
        with v.SaverDecryptor(ctx, vk_w, gabc[:N + 1], N, 16) as dec:
            msgs, _, dst = v.saver_decrypt_batch(ctx, dec, sk, agg)
        assert msgs.tolist() == [[votes.count(i) for i in range(N)]] and not dst.any()
        # a ballot that was invalid stays invalid for the same reason
        bad = Cc.copy(); bad[5] = g1_limbs(o.G1.neg(o.g1_from_limbs(bad[5])))
        _, reason0 = v.saver_verify_batch(ctx, ver, ct, rest, A, B, bad)
        ct3, abc3, _, _, st = v.saver_rerandomize_batch(ctx, rr, rnd, ct, (A, B, bad))
        verdict, reason = v.saver_verify_batch(ctx, ver, ct3, rest, *abc3)
        assert not st.any() and reason0.tolist() == [4 if k == 5 else 0 for k in range(12)] and reason.tolist() == reason0.tolist() and verdict[5] == 0
        verdict, reason = v.saver_verify_batch_screened(ctx, ver, ct3, rest, *abc3)
        assert reason.tolist() == reason0.tolist() and verdict.tolist() == [int(k != 5) for k in range(12)]
        # a batch in flight owns the context
        v.groth16_prove_batch_launch(ctx, dcs, kp.pk, W[:2], rand(2), rand(2))
        try:
            with pytest.raises(v.VspError, match=ERR_ARG + ".*in flight"):
                v.saver_rerandomize_batch(ctx, rr, rnd, ct, (A, B, Cc))
        finally:
            v.groth16_prove_batch_finish(ctx)
        assert np.array_equal(v.saver_rerandomize_batch(ctx, rr, rnd, ct, (A, B, Cc))[0], ct2)
    finally:
        tally.free(); rr.free()
        for h in handles:
            h.free()
