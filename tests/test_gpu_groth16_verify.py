"""GPU: vsp_groth16_verify_batch -- exact per-proof verdicts for proofs made by vsp_groth16_prove_batch, tampered members rejected one
by one, two members cross-checked with the oracle's groth16_verify."""
import numpy as np
import pytest

import bls12_381 as o
import pairing as pg
from conftest import I, L, fr_array, g1_limbs

import vote_saver_protocol_amd as v

pytestmark = pytest.mark.gpu
NC, NI, K = 48, 4, 66


@pytest.fixture(scope="module")
def proofs(ctx, cref):
    """a key for a system of 48 constraints with 4 public inputs, and 66 proofs of distinct witnesses"""
    gen = o.splitmix64(5)
    cs, wit0 = cref.R1CS.synth(NC, NI, 21)
    tox = fr_array([o.rand_fr(gen) for _ in range(5)])
    A_, B_, C_ = cs.export()
    dcs = v.R1CS(ctx, NC, NI, cs.num_vars, A_, B_, C_)
    kp = v.Keypair(ctx, dcs, tox)
    # boolean wires no product reads may take either value (test_gpu_prover.py); private ones only
    read = set()
    for j in range(NC):
        a, b, c = int(A_[1][j]), int(B_[1][j]), int(C_[1][j])
        if not (a == b == c):
            read.add(a); read.add(b)
    free = [int(C_[1][j]) for j in range(NC) if int(A_[1][j]) == int(B_[1][j]) == int(C_[1][j]) and int(C_[1][j]) not in read and int(C_[1][j]) > NI]
    assert len(free) >= 7, len(free)
    wits, rs, ss = [], [], []
    for k in range(K):
        w = wit0.copy()
        for t, idx in enumerate(free[:7]):
            w[idx - 1] = 0; w[idx - 1, 0] = (k >> t) & 1
        assert cs.is_satisfied(w)
        wits.append(w); rs.append(L(o.rand_fr(gen), 4)); ss.append(L(o.rand_fr(gen), 4))
    W = np.stack(wits)
    assert len({w.tobytes() for w in wits}) == K
    Rr, Ss = np.stack(rs), np.stack(ss)
    halves = [v.groth16_prove_batch(ctx, dcs, kp.pk, W[a:b], Rr[a:b], Ss[a:b]) for a, b in ((0, 64), (64, K))]      # a batch holds at most 64
    A, B, Cc = (np.concatenate([h[i] for h in halves]) for i in range(3))
    parts = {n: kp.part(n) for n in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "gamma_ABC_g1")}
    vk = v.VerifyingKey(ctx, parts["alpha_g1"][0], parts["beta_g2"][0], parts["gamma_g2"][0], parts["delta_g2"][0], parts["gamma_ABC_g1"])
    assert vk.n_abc == NI + 1
    yield dict(vk=vk, parts=parts, inputs=np.ascontiguousarray(W[:, :NI, :]), A=A, B=B, C=Cc)
    vk.free(); kp.free(); dcs.free(); cs.free()


def test_every_proof_is_accepted_and_two_agree_with_the_oracle(ctx, proofs):
    p = proofs
    assert v.groth16_verify_batch(ctx, p["vk"], p["inputs"], p["A"], p["B"], p["C"]).tolist() == [1] * K
    ovk = dict(alpha_g1=o.g1_from_limbs(p["parts"]["alpha_g1"][0]), beta_g2=o.g2_from_limbs(p["parts"]["beta_g2"][0]),
               gamma_g2=o.g2_from_limbs(p["parts"]["gamma_g2"][0]), delta_g2=o.g2_from_limbs(p["parts"]["delta_g2"][0]),
               gamma_ABC_g1=[o.g1_from_limbs(x) for x in p["parts"]["gamma_ABC_g1"]])
    for k in (0, 65):
        pub = [I(p["inputs"][k, i]) for i in range(NI)]
        assert pg.groth16_verify(ovk, pub, (o.g1_from_limbs(p["A"][k]), o.g2_from_limbs(p["B"][k]), o.g1_from_limbs(p["C"][k])))
    assert v.groth16_verify_batch(ctx, p["vk"], p["inputs"][5:6], p["A"][5:6], p["B"][5:6], p["C"][5:6]).tolist() == [1]      # n = 1


def test_tampered_members_are_rejected_and_only_they(ctx, proofs):
    p = proofs
    A, B, Cc, inputs = p["A"].copy(), p["B"].copy(), p["C"].copy(), p["inputs"].copy()
    A[0] = g1_limbs(o.G1.mul(o.g1_from_limbs(A[0]), 2))                       # A replaced by 2 A
    B[31] = p["B"][30]                                                         # another proof's B
    Cc[32] = g1_limbs(o.G1.neg(o.g1_from_limbs(Cc[32])))                       # C negated
    inputs[64, 1] = L((I(inputs[64, 1]) + 1) % o.R, 4)                         # one public input incremented
    A[65] = 0                                                                  # A = infinity
    want = [0 if k in (0, 31, 32, 64, 65) else 1 for k in range(K)]
    assert v.groth16_verify_batch(ctx, p["vk"], inputs, A, B, Cc).tolist() == want
    ctx.set_option("pairing_chunk", 20)
    try:
        assert v.groth16_verify_batch(ctx, p["vk"], inputs, A, B, Cc).tolist() == want
    finally:
        ctx.set_option("pairing_chunk", 1 << 14)


def test_malformed_members_are_rejected_alone(ctx, proofs):
    p = proofs
    A, B, Cc, inputs = p["A"].copy(), p["B"].copy(), p["C"].copy(), p["inputs"].copy()
    Cc[7, 6] ^= np.uint64(1)                                                   # C off the curve
    A[20, :6] = L(o.P, 6)                                                      # a coordinate equal to p
    inputs[40, 2] = L(I(inputs[40, 2]) + o.R, 4)                               # the same scalar, not reduced
    want = [0 if k in (7, 20, 40) else 1 for k in range(K)]
    assert v.groth16_verify_batch(ctx, p["vk"], inputs, A, B, Cc).tolist() == want
    assert v.groth16_verify_batch(ctx, p["vk"], p["inputs"], p["A"], p["B"], p["C"]).tolist() == [1] * K


def test_a_rerandomised_proof_still_verifies(ctx, proofs):
    """the proof part of vsp_saver_rerandomize with r' = 0: A' = z1 A, B' = B / z1 + z2 delta_g2, C' = C + z1 z2 A (the ciphertext is
    left as it is and takes no part in the plain Groth16 equation)"""
    p = proofs
    gen = o.splitmix64(77)
    gabc = p["parts"]["gamma_ABC_g1"]
    n = NI
    lib, ptr = ctx.lib, v.api._ptr
    rnd = fr_array([o.rand_fr(gen) for _ in range(3 * n + 2)])
    pk_w = np.zeros(lib.vsp_saver_pk_words(n), np.uint64); sk = np.zeros(4, np.uint64); vk_w = np.zeros(lib.vsp_saver_vk_words(n), np.uint64)
    some_g1 = g1_limbs(o.G1.mul(o.G1.gen, 11))                      # stands for delta_g1 / gamma_g1: only the ciphertext side reads them
    assert lib.vsp_saver_keygen(None, n, ptr(some_g1), ptr(some_g1.copy()), ptr(gabc), ptr(rnd), ptr(pk_w), ptr(sk), ptr(vk_w)) == 0
    spk = v.SaverPublicKey(ctx, pk_w, gabc, n)
    ct = np.stack([g1_limbs(o.G1.mul(o.G1.gen, 20 + i)) for i in range(n + 2)])
    rnd3 = np.zeros((3, 4), np.uint64); rnd3[1] = L(o.rand_fr(gen), 4); rnd3[2] = L(o.rand_fr(gen), 4)
    k = 9
    ct2, (A2, B2, C2), _ = v.saver_rerandomize(ctx, spk, p["parts"]["delta_g2"][0], rnd3, ct, (p["A"][k], p["B"][k], p["C"][k]))
    assert np.array_equal(ct2, ct) and not np.array_equal(A2, p["A"][k]) and not np.array_equal(B2, p["B"][k]) and not np.array_equal(C2, p["C"][k])
    assert v.groth16_verify_batch(ctx, p["vk"], p["inputs"][k:k + 1], A2, B2, C2).tolist() == [1]
    assert v.groth16_verify_batch(ctx, p["vk"], p["inputs"][k:k + 1], A2, p["B"][k], C2).tolist() == [0]
    spk.free()
