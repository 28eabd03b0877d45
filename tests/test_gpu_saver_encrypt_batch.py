"""GPU: ballots in batches -- vsp_saver_ciphertext_batch (the ciphertexts alone, k_saver_ct over the key's device tables) and
vsp_saver_encrypt_batch (the ciphertexts beside the batch prover's proofs, the SAVER term as a per-member addend of the assembly).

Every ciphertext is checked against the C oracle's saver_encrypt_ct and some against oracle/saver.py encrypt_ct; every proved member against
vsp_saver_encrypt on the same inputs and against the C oracle's prover with the SAVER term, in limbs and in proof bytes.  The crafted key
(delta_s_g1[0] = G_1, delta_sum_s_g1 = t_g1[0]) makes the additions of c_1 and psi meet equal operands, opposite ones and infinity."""
import ctypes as C

import numpy as np
import pytest

import bls12_381 as o
import saver as sv
from conftest import I, L, fr_array, g1_limbs
from test_gpu_batch_members import members, proof_bytes, verifying_key

import vote_saver_protocol_amd as v

pytestmark = pytest.mark.gpu
ERR_ARG = "vsp error -1"


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def saver_key(ctx, cref, n, seed, gabc=None, delta_g1=None, gamma_g1=None):
    """an election key over the given Groth16 points (or over multiples of the generator): (flat public key, secret key, verification key, gabc)"""
    gen = o.splitmix64(seed)
    if gabc is None:
        pts = cref.g1_batch_mul_gen(fr_array([o.rand_fr(gen) for _ in range(n + 3)]))
        gabc, delta_g1, gamma_g1 = np.ascontiguousarray(pts[:n + 1]), pts[n + 1], pts[n + 2]
    rnd = fr_array([o.rand_fr(gen) for _ in range(3 * n + 2)])
    pk_w, sk, vk_w = v.saver_generate_keypair(ctx, rnd, gabc, delta_g1, gamma_g1, n)
    return pk_w, sk, vk_w, np.ascontiguousarray(gabc[:n + 1])


def ballots(n, count, seed):
    """count members: message kinds one-hot, all-zero, full-size, R - 1 in turn, with r_enc 0, 1, R - 1, random changing every four members"""
    gen = o.splitmix64(seed)
    msgs, r_enc = np.zeros((count, n, 4), np.uint64), np.zeros((count, 4), np.uint64)
    for k in range(count):
        kind = k % 4
        if kind == 0:
            msgs[k, k % n] = L(1, 4)
        elif kind == 2:
            msgs[k] = fr_array([o.rand_fr(gen) for _ in range(n)])
        elif kind == 3:
            msgs[k] = L(o.R - 1, 4)
        r_enc[k] = L((0, 1, o.R - 1, o.rand_fr(gen))[(k // 4) % 4], 4)
    return msgs, r_enc


@pytest.fixture(scope="module")
def plain(ctx, cref):
    """per msg_size: the key, 67 members and the C oracle's ciphertext and addend of each, computed once"""
    out = {}
    for n in (3, 25):
        pk_w, _, _, gabc = saver_key(ctx, cref, n, 500 + n)
        msgs, r_enc = ballots(n, 67, 600 + n)
        want = np.stack([cref.saver_encrypt_ct(n, pk_w, gabc, msgs[k], r_enc[k]) for k in range(67)])
        add = np.stack([cref.g1_mul(pk_w[-12:], r_enc[k]) for k in range(67)])
        out[n] = dict(spk=v.SaverPublicKey(ctx, pk_w, gabc, n), pk_w=pk_w, gabc=gabc, msgs=msgs, r_enc=r_enc, want=want, add=add)
    yield out
    for e in out.values():
        e["spk"].free()


@pytest.mark.parametrize("n", [3, 25])
def test_ciphertext_batches_are_the_oracles(ctx, plain, n):
    """a. counts 1, 2 and 67 (more than one workgroup, the last one not full); ciphertexts, addends, blobs; two calls and small pieces give
    the same bytes; the host leg too"""
    e = plain[n]
    spk = e["spk"]
    assert spk.device_bytes == 0
    spk.upload(); spk.upload()
    assert spk.device_bytes >= (3 * n + 3) * 92160 and ctx.stat("saver_ct_table_ms") > 0
    for count in (1, 2, 67):
        ct, add, blobs = v.saver_ciphertext_batch(ctx, spk, e["msgs"][:count], e["r_enc"][:count])
        for k in range(count):
            assert np.array_equal(ct[k], e["want"][k]), (count, k)
            assert np.array_equal(add[k], e["add"][k]), (count, k)
            assert blobs[k] == v.g1_vector_to_blob(ct[k]), (count, k)
    assert ctx.stat("saver_ct_ms") > 0
    pk_o, gabc_o = sv.pk_from_words(e["pk_w"], n), [o.g1_from_limbs(x) for x in e["gabc"]]
    for k in (0, 6, 27):                                             # one-hot under r_enc = 0, full-size under r_enc = 1, R - 1 under R - 1
        want = sv.encrypt_ct(pk_o, gabc_o, [I(m) for m in e["msgs"][k]], I(e["r_enc"][k]))
        assert np.array_equal(ct[k], np.stack([g1_limbs(p) for p in want])), k
    whole = (ct, add, blobs)
    a, b = (v.saver_ciphertext_batch(ctx, spk, e["msgs"][s], e["r_enc"][s]) for s in (slice(0, 30), slice(30, 67)))
    assert np.array_equal(np.concatenate([a[0], b[0]]), ct) and np.array_equal(np.concatenate([a[1], b[1]]), add) and a[2] + b[2] == blobs
    for option, value in (("saver_ct_chunk", 16), ("saver_encrypt_gpu", 0)):
        ctx.set_option(option, value)
        try:
            got = v.saver_ciphertext_batch(ctx, spk, e["msgs"], e["r_enc"])
        finally:
            ctx.set_option(option, {"saver_ct_chunk": 1024, "saver_encrypt_gpu": 1}[option])
        assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1]) and got[2] == whole[2], option
    # ciphertexts alone
    ct2, none_a, none_b = v.saver_ciphertext_batch(ctx, spk, e["msgs"][:5], e["r_enc"][:5], addends=False, blobs=False)
    assert none_a is None and none_b is None and np.array_equal(ct2, ct[:5])


def test_crafted_key_equal_opposite_and_infinite_operands(ctx, cref):
    """b. msg_size 3, delta_s_g1[0] = G_1 and delta_sum_s_g1 = t_g1[0] (curve points: the key loads).  m_1 = r_enc: equal operands (a lane of
    c_1 adds a table entry to itself when r_enc has one digit); m_1 = R - r_enc: opposite operands, c_1 = infinity -- all-zero limbs and
    the blob's infinity record; r_enc = 0 with m = 0: every element infinity"""
    n = 3
    pk_w, _, _, gabc = saver_key(ctx, cref, n, 777)
    pk_w = pk_w.copy()
    pk_w[12:24] = gabc[1]
    o_sum = 12 + 24 * n + 24 * (n + 1)
    pk_w[o_sum:o_sum + 12] = pk_w[12 + 12 * n:24 + 12 * n]
    spk = v.SaverPublicKey(ctx, pk_w, gabc, n)
    pk_o, gabc_o = sv.pk_from_words(pk_w, n), [o.g1_from_limbs(x) for x in gabc]
    assert pk_o["delta_s_g1"][0] == gabc_o[1] and pk_o["delta_sum_s_g1"] == pk_o["t_g1"][0]
    gen = o.splitmix64(778)
    cases = []
    for r in (1, 15, 16, 1 << 252, o.rand_fr(gen)):
        cases += [([r, 5, 0], r), ([o.R - r, 5, 0], r)]
    cases += [([0, 0, 0], 0), ([0, 0, 0], 7), ([3, 0, 0], 0)]
    try:
        ct, add, blobs = v.saver_ciphertext_batch(ctx, spk, fr_array([m for msg, _ in cases for m in msg]).reshape(-1, n, 4), fr_array([r for _, r in cases]))
        for k, (msg, r) in enumerate(cases):
            want = sv.encrypt_ct(pk_o, gabc_o, msg, r)
            assert np.array_equal(ct[k], np.stack([g1_limbs(p) for p in want])), (msg, r)
            assert np.array_equal(add[k], g1_limbs(o.G1.mul(pk_o["gamma_inverse_sum_s_g1"], r))), (msg, r)
            assert blobs[k] == v.g1_vector_to_blob(ct[k])
            if msg[0] == r and r:
                assert want[1] == o.G1.mul(gabc_o[1], 2 * r % o.R)
            if msg[0] == o.R - r:
                assert want[1] is None and not ct[k, 1].any() and blobs[k][8 + 48:8 + 96] == o.g1_compress(None)
        assert not ct[len(cases) - 3].any() and not add[len(cases) - 3].any()
    finally:
        spk.free()


class Election:
    """c - e. nc = 900, ni = 30, msg_size 25, K = 8 distinct members (the zero witness, r = 0, s = 0, r = s = R - 1, two equal neighbours)
    under r_enc 0, 1, R - 1 and random ones; the oracle's ciphertexts and proofs, computed once"""
    def __init__(self, ctx, cref):
        n, nc, ni, K = 25, 900, 30, 8
        self.n, self.ni, self.K = n, ni, K
        gen = o.splitmix64(2525)
        self.cs, _ = cref.R1CS.synth(nc, ni, 25, ballot=(n, 3))
        tox = fr_array([o.rand_fr(gen) for _ in range(5)])
        self.ref = cref.Keypair(self.cs, tox)
        self.dcs = v.R1CS(ctx, nc, ni, self.cs.num_vars, *self.cs.export())
        self.kp = v.Keypair(ctx, self.dcs, tox)
        self.parts = {k: self.kp.part(k) for k in ("gamma_ABC_g1", "delta_g1", "gamma_g1", "alpha_g1", "beta_g2", "gamma_g2", "delta_g2")}
        self.pk_w, _, _, self.gabc = saver_key(ctx, cref, n, 2526, self.parts["gamma_ABC_g1"], self.parts["delta_g1"][0], self.parts["gamma_g1"][0])
        self.spk = v.SaverPublicKey(ctx, self.pk_w, self.gabc, n)
        self.W, self.R, self.S, _ = members(self.cs, K, 2527, ballot_size=n)
        self.Renc = fr_array([0, 1, o.R - 1] + [o.rand_fr(gen) for _ in range(K - 3)])
        self.W[3], self.R[3], self.S[3], self.Renc[3] = self.W[4], self.R[4], self.S[4], self.Renc[4]        # equal neighbours
        self.M = np.ascontiguousarray(self.W[:, :n])
        self.want_ct = np.stack([cref.saver_encrypt_ct(n, self.pk_w, self.gabc, self.M[k], self.Renc[k]) for k in range(K)])
        self.want = [self.ref.prove(self.W[k], self.R[k], self.S[k], P1=self.pk_w[-12:], r_enc=self.Renc[k]) for k in range(K)]
        self.want_bytes = [proof_bytes(*w) for w in self.want]
        self.plain_bytes = [proof_bytes(*self.ref.prove(self.W[k], self.R[k], self.S[k])) for k in range(K)]

    def batch(self, ctx, pick=slice(None)):
        return v.saver_encrypt_batch(ctx, self.spk, self.dcs, self.kp.pk, self.M[pick], self.W[pick], self.Renc[pick], self.R[pick], self.S[pick])

    def check(self, out, pick=slice(None)):
        ct, (A, B, Cc), proofs, blobs = out
        idx = pick if isinstance(pick, list) else list(range(self.K))[pick]
        for j, k in enumerate(idx):
            assert np.array_equal(ct[j], self.want_ct[k]), k
            assert np.array_equal(A[j], self.want[k][0]) and np.array_equal(B[j], self.want[k][1]) and np.array_equal(Cc[j], self.want[k][2]), k
            assert proofs[j] == self.want_bytes[k] and blobs[j] == v.g1_vector_to_blob(self.want_ct[k]), k

    def free(self):
        for h in (self.spk, self.kp, self.dcs, self.ref, self.cs):
            h.free()


@pytest.fixture(scope="module")
def election(ctx, cref):
    e = Election(ctx, cref)
    yield e
    e.free()


def test_proved_batch_members_equal_the_single_call_and_the_oracle(ctx, election):
    """c."""
    e = election
    assert len(set(e.want_bytes)) == e.K - 1
    out = e.batch(ctx)
    e.check(out)
    assert ctx.stat("saver_encrypt_batches") >= 1
    for k in range(e.K):
        ct, (A, B, Cc), proof = v.saver_encrypt(ctx, e.spk, e.dcs, e.kp.pk, e.M[k], e.W[k], e.Renc[k], e.R[k], e.S[k])
        assert np.array_equal(ct, out[0][k]) and proof == out[2][k], k
        assert np.array_equal(A, out[1][0][k]) and np.array_equal(B, out[1][1][k]) and np.array_equal(Cc, out[1][2][k]), k
    ver = v.SaverVerifier(ctx, e.pk_w, e.parts["alpha_g1"][0], e.parts["beta_g2"][0], e.parts["gamma_g2"][0], e.parts["delta_g2"][0], e.parts["gamma_ABC_g1"], e.n)
    try:
        verdict, reason = v.saver_verify_batch(ctx, ver, out[0], np.ascontiguousarray(e.W[:, e.n:e.ni]), *out[1])
        assert verdict.tolist() == [1] * e.K and not reason.any()
    finally:
        ver.free()
    pts = lambda rows: [o.g1_from_limbs(x) for x in rows]
    assert sv.verify_encryption(sv.pk_from_words(e.pk_w, e.n), verifying_key(e.kp), pts(out[0][0]),
                                (o.g1_from_limbs(out[1][0][0]), o.g2_from_limbs(out[1][1][0]), o.g1_from_limbs(out[1][2][0])), [I(x) for x in e.W[0, e.n:e.ni]])
    e.check(e.batch(ctx, slice(None, None, -1)), slice(None, None, -1))
    ctx.set_option("saver_encrypt_gpu", 0)
    try:
        e.check(e.batch(ctx))
    finally:
        ctx.set_option("saver_encrypt_gpu", 1)
    # the addend does not stick
    assert v.groth16_prove_batch(ctx, e.dcs, e.kp.pk, e.W, e.R, e.S)[3] == e.plain_bytes


def test_two_contexts_in_flight_over_one_key(ctx, election):
    """d."""
    e = election
    other = v.Context(ctx.device)
    try:
        a, b = slice(0, 5), slice(3, 8)
        v.saver_encrypt_batch_launch(ctx, e.spk, e.dcs, e.kp.pk, e.M[a], e.W[a], e.Renc[a], e.R[a], e.S[a])
        v.saver_encrypt_batch_launch(other, e.spk, e.dcs, e.kp.pk, e.M[b], e.W[b], e.Renc[b], e.R[b], e.S[b])
        e.check(v.saver_encrypt_batch_finish(ctx), a)
        e.check(v.saver_encrypt_batch_finish(other), b)
    finally:
        other.close()


def test_refusals_name_the_member_and_leave_the_context_usable(ctx, election):
    """e."""
    e = election
    launch = lambda M=e.M, Renc=e.Renc: v.saver_encrypt_batch_launch(ctx, e.spk, e.dcs, e.kp.pk, M, e.W, Renc, e.R, e.S)
    M = e.M.copy(); M[5, 2] = L(I(M[5, 2]) + 1, 4)
    with pytest.raises(v.VspError, match=ERR_ARG + ".*member 5 differs"):
        launch(M=M)
    Renc = e.Renc.copy(); Renc[2] = L(o.R, 4)
    with pytest.raises(v.VspError, match=ERR_ARG + ".*r_enc of member 2"):
        launch(Renc=Renc)
    with pytest.raises(v.VspError, match=ERR_ARG + ".*member 2"):
        v.saver_ciphertext_batch(ctx, e.spk, e.M, Renc)
    z12 = np.zeros(12, np.uint64)
    for count in (0, 65):
        rc = ctx.lib.vsp_saver_encrypt_batch_launch(ctx.h, e.spk.h, e.dcs.h, e.kp.pk.h, _p(e.M), _p(e.W), count, _p(e.Renc), _p(e.R), _p(e.S))
        assert rc == -1 and "outside 1..64" in ctx.last_error(), count
    assert ctx.lib.vsp_saver_encrypt_batch_finish(ctx.h, None, None, None, None, None, None) == -1 and "no batch" in ctx.last_error()
    with pytest.raises(v.VspError, match=ERR_ARG):
        v.saver_encrypt_batch_finish(ctx)
    assert ctx.lib.vsp_saver_ciphertext_batch(ctx.h, e.spk.h, _p(e.M), _p(e.Renc), 1, None, _p(z12), None) == -1
    e.check(e.batch(ctx))
    # one unsatisfying member: the wire its last row defines is off by two (a bit is no bit any more, a product no product), its message untouched
    W = e.W.copy(); W[6, -1] = L((I(W[6, -1]) + 2) % o.R, 4)
    status, _, _ = e.dcs.check(ctx, W)
    assert status.tolist() == [0] * 6 + [2, 0]
    ctx.set_option("prove_check_witness", 1)
    try:
        with pytest.raises(v.Unsatisfied) as x:
            v.saver_encrypt_batch(ctx, e.spk, e.dcs, e.kp.pk, e.M, W, e.Renc, e.R, e.S)
        assert x.value.status.tolist() == [0] * 6 + [2, 0]
        ct, (A, B, Cc), proofs, blobs = x.value.results
        assert not ct[6].any() and not A[6].any() and not B[6].any() and not Cc[6].any() and proofs[6] == bytes(192) and blobs[6] == bytes(len(blobs[6]))
        keep = [0, 1, 2, 3, 4, 5, 7]
        e.check((ct[keep], (A[keep], B[keep], Cc[keep]), [proofs[k] for k in keep], [blobs[k] for k in keep]), keep)
        e.check(e.batch(ctx))                                        # all good with the check on
    finally:
        ctx.set_option("prove_check_witness", 0)
    assert v.groth16_prove_batch(ctx, e.dcs, e.kp.pk, e.W, e.R, e.S)[3] == e.plain_bytes


def test_six_ballots_from_one_batch_to_the_decrypted_tally(ctx, cref):
    """f. msg_size 3: the batch's blobs through vsp_tally_add_blobs and vsp_saver_decrypt_batch; the counts are the votes"""
    n, nc, ni = 3, 60, 5
    votes = [0, 2, 2, 1, 2, 0]
    gen = o.splitmix64(333)
    tox = fr_array([o.rand_fr(gen) for _ in range(5)])
    systems = [cref.R1CS.synth(nc, ni, 33, ballot=(n, vote)) for vote in votes]      # the same system, another ballot
    cs = systems[0][0]
    dcs = v.R1CS(ctx, nc, ni, cs.num_vars, *cs.export())
    kp = v.Keypair(ctx, dcs, tox)
    pk_w, sk, vk_w, gabc = saver_key(ctx, cref, n, 334, kp.part("gamma_ABC_g1"), kp.part("delta_g1")[0], kp.part("gamma_g1")[0])
    spk = v.SaverPublicKey(ctx, pk_w, gabc, n)
    W = np.stack([w for _, w in systems])
    rnd = lambda: fr_array([o.rand_fr(gen) for _ in votes])
    tally = v.Tally(ctx, n + 2)
    try:
        assert [[I(x) for x in w[:n]] for w in W] == [[int(i == vote) for i in range(n)] for vote in votes]
        ct, _, _, blobs = v.saver_encrypt_batch(ctx, spk, dcs, kp.pk, np.ascontiguousarray(W[:, :n]), W, rnd(), rnd(), rnd())
        status, accepted = tally.add_blobs(blobs)
        assert accepted == len(votes) and not status.any()
        agg, _ = tally.result()
        with v.SaverDecryptor(ctx, vk_w, gabc, n, 16) as dec:
            msgs, _, st = v.saver_decrypt_batch(ctx, dec, sk, agg)
        assert msgs.tolist() == [[2, 1, 3]] and not st.any()
    finally:
        tally.free(); spk.free(); kp.free(); dcs.free()
        for c, _ in systems:
            c.free()
