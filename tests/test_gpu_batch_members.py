"""GPU: batches whose members differ.  Every member of a batch owns its slice of the device work -- its row of the CSR products, its three
slices of the strided 3K-vector transforms and their scratch, its bucket sets in the batched multi-exponentiations -- so every member is
checked against a reference of its own: the C oracle's prover, the single-call proof, the pairing equation, or for the multi-exponentiations
(sum_i k_i s_i) G over bases k_i G.  A batch that gave some member another member's data passes none of these."""
import numpy as np
import pytest

import bls12_381 as o
from conftest import I, L, fr_array, fr_ints_fast, g1_limbs, g2_limbs, rand_fr_array

import vote_saver_protocol_amd as v

pytestmark = pytest.mark.gpu

OPTIONS = ((None, None), ("prove_batch_share_plan", 0), ("witness_map_batched", 0), ("msm_dimbits", 0), ("msm_dimbits", 1))
DEFAULTS = {"prove_batch_share_plan": 1, "witness_map_batched": 1, "msm_dimbits": -1}


def members(cs, K, seed, ballot_size=0):
    """K distinct (witness, r, s) of one system: resampled witnesses under random (r, s), with the zero member at 1, r = 0 at 2, two equal
    members at K/2 and K/2 + 1, s = 0 at K - 3 and r = s = R - 1 at K - 1.  ballot_size: member k votes k mod ballot_size.
    -> (W [K, num_vars, 4], R [K, 4], S [K, 4], index of the zero member)"""
    gen = o.splitmix64(seed)
    ws, rs, ss = [], [], []
    for k in range(K):
        ws.append(cs.resample_witness(seed * 1000 + k, ballot=(ballot_size, k % ballot_size) if ballot_size else None, zero=k == 1))
        rs.append(L(o.rand_fr(gen), 4)); ss.append(L(o.rand_fr(gen), 4))
    ws[K // 2 + 1], rs[K // 2 + 1], ss[K // 2 + 1] = ws[K // 2], rs[K // 2], ss[K // 2]
    rs[2] = L(0, 4)
    ss[K - 3] = L(0, 4)
    rs[K - 1] = ss[K - 1] = L(o.R - 1, 4)
    return np.stack(ws), np.stack(rs), np.stack(ss), 1


def proof_bytes(A, B, Cc):
    return o.g1_compress(o.g1_from_limbs(A)) + o.g2_compress(o.g2_from_limbs(B)) + o.g1_compress(o.g1_from_limbs(Cc))


def oracle_key_on_device(ctx, kp):
    q = [ctx.upload_bases(kp.part(n), g) for n, g in (("A_query", 1), ("B_query_g1", 1), ("B_query_g2", 2), ("H_query", 1), ("L_query", 1))]
    pk = v.ProvingKey(ctx, kp.part("alpha_g1")[0], kp.part("beta_g1")[0], kp.part("beta_g2")[0], kp.part("delta_g1")[0], kp.part("delta_g2")[0], *q)
    return pk, q


def set_options(ctx, name, value):
    for k, d in DEFAULTS.items():
        ctx.set_option(k, d)
    if name is not None:
        ctx.set_option(name, value)


def verifying_key(kp):
    return dict(alpha_g1=o.g1_from_limbs(kp.part("alpha_g1")[0]), beta_g2=o.g2_from_limbs(kp.part("beta_g2")[0]),
                gamma_g2=o.g2_from_limbs(kp.part("gamma_g2")[0]), delta_g2=o.g2_from_limbs(kp.part("delta_g2")[0]),
                gamma_ABC_g1=[o.g1_from_limbs(x) for x in kp.part("gamma_ABC_g1")])


@pytest.mark.parametrize("nc,ni,K,m,tables", [(10, 2, 64, 16, False), (2000, 30, 32, 2048, True), (4000, 5, 64, 4096, True),
                                              (5000, 3, 16, 5120, False)])
def test_every_member_of_a_batch_against_the_oracle(ctx, cref, nc, ni, K, m, tables):
    """K distinct members -- resampled witnesses, the zero witness, two equal neighbours, r = 0, s = 0, r = s = R - 1 -- proved in one batch:
    each member's A, B, C equal the C oracle's proof and its bytes equal vsp_groth16_prove's, over the oracle's key and over a generated key
    with 14-bit tables on all five queries, under each batch option; the reversed batch gives the reversed proofs; and a member's proof
    does not depend on its neighbours (the batch's digit census, which picks the window, is a mean over the members)."""
    gen = o.splitmix64(31 * nc + K)
    cs, _ = cref.R1CS.synth(nc, ni, nc + K)
    assert cs.m == m and cs.is_step == (m == 5120)
    tox = fr_array([o.rand_fr(gen) for _ in range(5)])
    ref = cref.Keypair(cs, tox)
    dcs = v.R1CS(ctx, nc, ni, cs.num_vars, *cs.export())
    W, R, S, _ = members(cs, K, nc + K)
    want, seen = [], {}
    for k in range(K):
        key = (W[k].tobytes(), R[k].tobytes(), S[k].tobytes())
        if key not in seen:
            seen[key] = ref.prove(W[k], R[k], S[k])
        want.append(seen[key])
    want_bytes = [proof_bytes(*e) for e in want]
    assert len(set(want_bytes)) == K - 1                          # only the equal neighbours share a proof
    pk, q = oracle_key_on_device(ctx, ref)
    keys = [("oracle key", pk)]
    if tables:
        kpt = v.Keypair(ctx, dcs, tox, precompute=17, precompute_window=14)
        keys.append(("14-bit tables", kpt.pk))
    for k in range(K):
        sA, sB, sC, sp = v.groth16_prove(ctx, dcs, pk, W[k], R[k], S[k])
        assert np.array_equal(sA, want[k][0]) and np.array_equal(sB, want[k][1]) and np.array_equal(sC, want[k][2]) and sp == want_bytes[k], k
    dense = rand_fr_array(K * cs.num_vars, nc + 1).reshape(K, cs.num_vars, 4)
    j = K // 3
    try:
        for kname, key in keys:
            for name, value in OPTIONS:
                set_options(ctx, name, value)
                A, B, Cc, proofs = v.groth16_prove_batch(ctx, dcs, key, W, R, S)
                for k in range(K):
                    assert np.array_equal(A[k], want[k][0]) and np.array_equal(B[k], want[k][1]) and np.array_equal(Cc[k], want[k][2]), (kname, name, value, k)
                    assert proofs[k] == want_bytes[k], (kname, name, value, k)
            set_options(ctx, None, None)
            assert v.groth16_prove_batch(ctx, dcs, key, W[::-1], R[::-1], S[::-1])[3] == want_bytes[::-1], kname
            # member 0 alone, among K - 1 dense neighbours (uniform field elements on every wire), among K - 1 zero neighbours
            assert v.groth16_prove_batch(ctx, dcs, key, W[:1], R[:1], S[:1])[3] == want_bytes[:1], kname
            for nb in (dense, np.zeros_like(dense)):
                Wn = nb.copy(); Wn[j] = W[0]
                Rn = fr_array([o.rand_fr(gen) for _ in range(K)]); Rn[j] = R[0]
                Sn = fr_array([o.rand_fr(gen) for _ in range(K)]); Sn[j] = S[0]
                assert v.groth16_prove_batch(ctx, dcs, key, Wn, Rn, Sn)[3][j] == want_bytes[0], (kname, bool(nb.any()))
    finally:
        set_options(ctx, None, None)
    if tables:
        kpt.free()
    pk.free(); [x.free() for x in q]; dcs.free(); ref.free(); cs.free()


def test_production_shape_batches_of_distinct_ballots(ctx, cref):
    """The benchmark's circuit (2^16 - 32 constraints, 30 public inputs, a one-hot ballot in the first 25), a different vote per member:
    batches of 32 over a plain generated key and over one with 14-bit tables on all five queries, and of 64 over the plain key.  Every
    member equals its single-call proof; members 0 and K - 1 and the zero member satisfy the pairing equation with their own public
    inputs, member 0's proof fails with member 1's; the benchmark's ring of three contexts over the table key, each launch a different batch,
    gives what the blocking calls give."""
    import pairing as pg
    ni = 30
    nc = (1 << 16) - ni - 2
    gen = o.splitmix64(1616)
    cs, _ = cref.R1CS.synth(nc, ni, 40, ballot=(25, 3))
    tox = fr_array([o.rand_fr(gen) for _ in range(5)])
    dcs = v.R1CS(ctx, nc, ni, cs.num_vars, *cs.export())
    assert dcs.m == 1 << 16
    W, R, S, z = members(cs, 64, 16, ballot_size=25)
    kpp = v.Keypair(ctx, dcs, tox, precompute=False)
    kpt = v.Keypair(ctx, dcs, tox, precompute=17, precompute_window=14)
    single = [v.groth16_prove(ctx, dcs, kpp.pk, W[k], R[k], S[k]) for k in range(64)]
    assert len({x[3] for x in single}) == 63
    for k in (0, 5, 63):
        assert v.groth16_prove(ctx, dcs, kpt.pk, W[k], R[k], S[k])[3] == single[k][3], k
    batch = {}
    for kname, key, lo, K in (("plain", kpp, 0, 32), ("tables", kpt, 32, 32), ("plain", kpp, 0, 64)):
        A, B, Cc, proofs = v.groth16_prove_batch(ctx, dcs, key.pk, W[lo:lo + K], R[lo:lo + K], S[lo:lo + K])
        assert proofs == [single[lo + k][3] for k in range(K)], (kname, K)
        batch[(kname, K)] = (A, B, Cc)
    vk = verifying_key(kpp)
    A, B, Cc = batch[("plain", 64)]
    pub = lambda k: [I(W[k][i]) for i in range(ni)]
    proof = lambda k: (o.g1_from_limbs(A[k]), o.g2_from_limbs(B[k]), o.g1_from_limbs(Cc[k]))
    for k in (0, 63, z):
        assert pg.groth16_verify(vk, pub(k), proof(k)), k
    assert not pg.groth16_verify(vk, pub(1), proof(0))
    # the ring: ONE host thread, three contexts, launch i on context i % 3 with batch i % 4
    picks = [np.arange(0, 32), np.arange(32, 64), np.arange(16, 48), np.arange(31, -1, -1)]
    expect = [v.groth16_prove_batch(ctx, dcs, kpt.pk, W[p], R[p], S[p])[3] for p in picks]
    for e, p in zip(expect, picks):
        assert e == [single[k][3] for k in p]
    ring = [ctx, v.Context(ctx.device), v.Context(ctx.device)]
    try:
        total = 8
        for i in range(total + 3):
            c = ring[i % 3]
            if i >= 3:
                assert v.groth16_prove_batch_finish(c)[3] == expect[(i - 3) % 4], i - 3
            if i < total:
                p = picks[i % 4]
                v.groth16_prove_batch_launch(c, dcs, kpt.pk, W[p], R[p], S[p])
    finally:
        for c in ring[1:]:
            c.close()
    kpt.free(); kpp.free(); dcs.free(); cs.free()


MSM_KINDS = ("uniform", "boolean", "zero", "equal", "edges", "single")


def msm_vectors(K, n, seed):
    """K scalar vectors of n, the kinds in turn: uniform, 90 % boolean, zero, all equal, edge values (R - 1, R - 2, R - 3, 0, 1), one nonzero"""
    rng = np.random.default_rng(seed)
    vecs = rand_fr_array(K * n, seed).reshape(K, n, 4)
    for k in range(K):
        kind, ss = MSM_KINDS[k % len(MSM_KINDS)], vecs[k]
        if kind == "boolean":
            m = rng.random(n) < 0.9; ss[m] = 0; ss[m, 0] = rng.integers(0, 2, size=int(m.sum()), dtype=np.uint64)
        elif kind == "zero":
            ss[:] = 0
        elif kind == "equal":
            ss[:] = ss[k]
        elif kind == "edges":
            for i, e in enumerate((o.R - 1, o.R - 2, o.R - 3, 0, 1)):
                ss[i::5] = L(e, 4)
        elif kind == "single":
            one = ss[(7919 * k) % (n - 40) + 3].copy(); ss[:] = 0; ss[(7919 * k) % (n - 40) + 3] = one
    return vecs


@pytest.mark.parametrize("group,Ks", [(1, (32, 64)), (2, (32,))])
def test_batched_msm_members_at_2p16_by_the_discrete_log_identity(ctx, cref, group, Ks):
    """vsp_msm_resident_batch at the prover's size: bases k_i G made on the GPU, so member k of a batch must be (sum_i k_i s_ki mod R) G --
    checked member by member for K = 32 and 64 (G1) and 32 (G2), over all 2^16 bases and over 2^16 - 31 of them from the fourth on, with
    plain bases and 14-bit tables of window multiples, with and without the endomorphism split.  The members are of six kinds: uniform,
    90 % boolean, zero, all equal, edge values and a single nonzero scalar."""
    n, first, cnt = 1 << 16, 3, (1 << 16) - 31
    ks = rand_fr_array(n, 900 + group)
    kmax = max(Ks)
    vecs = msm_vectors(kmax, n, 950 + group)
    ki = np.array(fr_ints_fast(ks), dtype=object)
    expo = {}
    for k in range(kmax):
        si = np.array(fr_ints_fast(vecs[k]), dtype=object)
        expo[(0, k)] = int(np.dot(ki, si)) % o.R
        expo[(first, k)] = int(np.dot(ki[first:first + cnt], si[:cnt])) % o.R
    gen_pt = g1_limbs(o.G1.gen) if group == 1 else g2_limbs(o.G2.gen)
    mul = cref.g1_mul if group == 1 else cref.g2_mul
    want = {key: mul(gen_pt, L(e, 4)) for key, e in expo.items()}
    d_k = ctx.to_device(ks); d_s = ctx.to_device(vecs.reshape(-1, 4))
    d_b = v.fixed_base_mul(ctx, d_k, n, group)
    try:
        for glv in (1, 0):
            ctx.set_option("msm_glv", glv)
            for tables in (False, True):
                B = ctx.bases_from_device(d_b, n, group)
                if tables:
                    B.precompute(14, split=bool(glv))
                try:
                    for K in Ks:
                        for f, c in ((0, n), (first, cnt)):
                            got, inf = B.msm_batch(d_s, K, n=c, first=f, stride=n)
                            for k in range(K):
                                assert np.array_equal(got[k], want[(f, k)]), (group, glv, tables, K, f, k, MSM_KINDS[k % len(MSM_KINDS)])
                                assert bool(inf[k]) == (expo[(f, k)] == 0), (group, glv, tables, K, f, k)
                finally:
                    B.free()
    finally:
        ctx.set_option("msm_glv", 1)
        ctx.dfree(d_b); ctx.dfree(d_k); ctx.dfree(d_s)
