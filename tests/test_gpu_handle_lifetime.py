"""GPU: every handle kind, a context and the creates that fail give back the memory they took.

The library counts its live device and pinned allocations (vsp_get_stat "device_allocations_live" / "pinned_allocations_live", over the
whole process).  A handle is created, used once so that whatever it grows on first use exists, and freed -- twice: the first round lets
the shared context grow the workspaces the calls need (they stay with the context), the second must leave both counts where it found
them.  The last test asks the driver instead of the counters (hipMemGetInfo)."""
import ctypes as C
import random

import numpy as np
import pytest

import bls12_381 as o
import dlog_election as de
import jubjub_model as jm
import vote_saver_protocol_amd as v
from conftest import fr_array, rand_fr_array

pytestmark = pytest.mark.gpu
N_MSG = 2                                                           # msg_size throughout
NC, NI = 16, 3                                                      # the constraint system: 16 constraints, msg_size + 1 inputs


def counts(ctx):
    return int(ctx.stat("device_allocations_live")), int(ctx.stat("pinned_allocations_live"))


def returns_to_baseline(ctx, cycle):
    """cycle() creates, uses and frees: once to let the context grow its workspaces, once more between two readings of the counters"""
    cycle()
    before = counts(ctx)
    cycle()
    assert counts(ctx) == before


def fails_clean(ctx, create, text):
    """create() raises VspError with `text` as the context's error; the second time between two readings of the counters"""
    for measured in (False, True):
        before = counts(ctx)
        with pytest.raises(v.VspError):
            create()
        assert ctx.last_error() == text
        if measured:
            assert counts(ctx) == before


class World:
    """what the handles are made of, computed once: points, a constraint system with its keys, a SAVER key over them, an election of
    known logs (tests/dlog_election.py) with ballots as blobs, Pedersen generators and registered keys"""

    def __init__(self, ctx, cref):
        self.g1 = cref.g1_batch_mul_gen(rand_fr_array(1024, 1))
        self.g2 = cref.g2_batch_mul_gen(rand_fr_array(1024, 2))
        self.scalars = rand_fr_array(1024, 3)
        self.cs, self.wit = cref.R1CS.synth(NC, NI, 7)
        self.csr = self.cs.export()
        self.tox = rand_fr_array(5, 8)
        self.ref = cref.Keypair(self.cs, self.tox)
        self.gabc = self.ref.part("gamma_ABC_g1")
        self.pk_w, self.sk, self.vk_w = v.saver_generate_keypair(ctx, rand_fr_array(3 * N_MSG + 2, 9), self.gabc, self.ref.part("delta_g1")[0],
                                                                 self.ref.part("gamma_g1")[0], N_MSG)
        self.delta_g2 = self.ref.part("delta_g2")[0]
        self.W = np.stack([self.wit, self.cs.resample_witness(1)])
        self.rnd = rand_fr_array(6, 10).reshape(3, 2, 4)            # r_enc, r, s of two members
        rng = de.rng(11)
        self.el = de.Election(rng, N_MSG, 1)
        members = [de.make_ballot(self.el, [de.nonzero(rng) for _ in range(N_MSG + 1)], [1000 + k], rng) for k in range(6)]
        b = de.ballot_batch(self.el, members)
        assert b["want"] == [0] * 6
        self.ballots = b
        self.ct_blobs = [v.g1_vector_to_blob(b["ct"][k]) for k in range(6)]
        self.pr_blobs = [v.g1_compress(b["A"][k]) + v.g2_compress(b["B"][k]) + v.g1_compress(b["C"][k]) for k in range(6)]
        self.in_blobs = [v.fr_vector_to_blob(b["rest"][k]) for k in range(6)]
        self.gens = np.array([jm.point_words(g) for g in jm.generators(3)], np.uint64)
        prng = random.Random(12)
        self.eid = np.array(jm.message_words([prng.getrandbits(1) for _ in range(8)]), np.uint64)
        self.sks = np.array([jm.words(prng.getrandbits(255)) for _ in range(8)], np.uint64).reshape(-1, 4)

    def r1cs(self, ctx):
        return v.R1CS(ctx, NC, NI, self.cs.num_vars, *self.csr)

    def verifier(self, ctx):
        k = self.el.key
        return v.SaverVerifier(ctx, self.el.pk_words, k.alpha, k.beta, k.gamma, k.delta, k.gamma_abc, N_MSG)

    def free(self):
        self.ref.free(); self.cs.free()


@pytest.fixture(scope="module")
def w(ctx, cref):
    world = World(ctx, cref)
    yield world
    world.free()


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("how", ["plain", "precompute", "split"])
def test_bases(ctx, w, group, how):
    pts = w.g1 if group == 1 else w.g2
    d_scalars = ctx.to_device(w.scalars)                            # the caller's memory: not counted

    def cycle():
        b = ctx.upload_bases(pts, group)
        if how != "plain":
            b.precompute(window_bits=8, split=how == "split")       # the table takes the place of the points
        b.msm(d_scalars)
        b.free()
    try:
        returns_to_baseline(ctx, cycle)
    finally:
        ctx.dfree(d_scalars)


def test_r1cs(ctx, w):
    def cycle():
        cs = w.r1cs(ctx)
        assert cs.is_satisfied(ctx, w.wit)
        cs.free()
    returns_to_baseline(ctx, cycle)


def test_step_domain(ctx):
    a = rand_fr_array(96, 20)

    def cycle():
        dom = v.make_evaluation_domain(ctx, 96)
        assert dom.kind == "step_radix2"                            # the kind with a table of coset divisors
        dom.divide_by_z_on_coset(a)
        dom.fft(a)
        dom.free()
    returns_to_baseline(ctx, cycle)


def test_keypair_generated_and_from_blob(ctx, w):
    r, s = w.rnd[1][0], w.rnd[2][0]
    cs = w.r1cs(ctx)
    expect = [None]

    def generated():
        kp = v.Keypair(ctx, cs, w.tox)
        expect[0] = v.groth16_prove(ctx, cs, kp.pk, w.wit, r, s)[3]
        blob = kp.to_blob()
        kp.free()
        return blob
    try:
        returns_to_baseline(ctx, generated)
        blob = generated()

        def loaded():
            kp = v.Keypair.from_blob(ctx, blob)
            assert v.groth16_prove(ctx, cs, kp.pk, w.wit, r, s)[3] == expect[0]
            kp.free()
        returns_to_baseline(ctx, loaded)
    finally:
        cs.free()


def test_verifying_key(ctx, w):
    k = w.el.key
    rng = de.rng(30)
    p = de.proof_batch(k, [de.make_proof(k, [rng.randrange(o.R) for _ in range(k.n_abc - 1)], rng)])

    def cycle():
        vk = v.VerifyingKey(ctx, k.alpha, k.beta, k.gamma, k.delta, k.gamma_abc)
        assert v.groth16_verify_batch(ctx, vk, p["inputs"], p["A"], p["B"], p["C"]).tolist() == [1]
        vk.free()
    returns_to_baseline(ctx, cycle)


def test_saver_verifier(ctx, w):
    b = w.ballots

    def cycle():
        ver = w.verifier(ctx)
        verdict, _ = v.saver_verify_batch(ctx, ver, b["ct"][:2], b["rest"][:2], b["A"][:2], b["B"][:2], b["C"][:2])
        assert verdict.tolist() == [1, 1]
        ver.free()
    returns_to_baseline(ctx, cycle)


def test_saver_public_key_rerandomizer_and_decryptor(ctx, w, cref):
    msgs = fr_array([3, 5, 0, 9]).reshape(2, N_MSG, 4)
    z = fr_array([o.rand_fr(o.splitmix64(40)) for _ in range(6)]).reshape(2, 3, 4)          # r', z1 (not zero), z2 of two members
    g1 = w.g1[:2 * (N_MSG + 4)].reshape(2, N_MSG + 4, 12)
    ct_in, A, B, Cc = np.ascontiguousarray(g1[:, :N_MSG + 2]), np.ascontiguousarray(g1[:, N_MSG + 2]), w.g2[:2], np.ascontiguousarray(g1[:, N_MSG + 3])

    def cycle():
        spk = v.SaverPublicKey(ctx, w.pk_w, w.gabc[:N_MSG + 1], N_MSG)
        spk.upload()
        assert spk.device_bytes > 0
        ct, _, _ = v.saver_ciphertext_batch(ctx, spk, msgs, w.rnd[0])
        rr = v.SaverRerandomizer(ctx, spk, w.delta_g2)
        assert not v.saver_rerandomize_batch(ctx, rr, z, ct_in, (A, B, Cc))[4].any()
        dec = v.SaverDecryptor(ctx, w.vk_w, w.gabc[:N_MSG + 1], N_MSG, 1 << 10)
        got, _, status = v.saver_decrypt_batch(ctx, dec, w.sk, ct)
        assert got.tolist() == [[3, 5], [0, 9]] and not status.any()
        dec.free(); rr.free(); spk.free()
    returns_to_baseline(ctx, cycle)


def test_ballot_box_that_grew_its_table(ctx, w):
    ver = w.verifier(ctx)
    expected = de._fr([0])

    def cycle():
        ctx.set_option("ballot_box_table_bits", 2)                  # four slots: six serials do not fit in half of them
        try:
            box = v.BallotBox(ctx, ver, expected, [v.api.SERIAL])
        finally:
            ctx.set_option("ballot_box_table_bits", 16)
        grown = ctx.stat("ballot_box_grown")
        verdict = box.receive_blobs(w.ct_blobs, w.pr_blobs, w.in_blobs)[0]
        assert verdict.tolist() == [1] * 6 and ctx.stat("ballot_box_grown") > grown
        box.free()
    try:
        returns_to_baseline(ctx, cycle)
    finally:
        ver.free()


def test_pedersen_registry_and_vote_circuit(ctx, w):
    def cycle():
        ped = v.Pedersen(ctx, w.gens)
        pks = v.pedersen_hash_batch(ctx, ped, w.sks, 255)
        reg = v.Registry.build(ctx, ped, pks, 3)
        loaded = v.Registry.from_blob(ctx, ped, reg.to_blob(), 3)
        assert np.array_equal(loaded.root(), reg.root())
        circ = v.VoteCircuit(ctx, ped, N_MSG, 8, 3)
        _, _, status = circ.witness_batch_device(reg, w.eid, w.sks[:2], [0, 1], [0, 1])
        assert not status.any()
        circ.witness_release()
        circ.free(); loaded.free(); reg.free(); ped.free()
    returns_to_baseline(ctx, cycle)


def test_tally(ctx, w):
    def cycle():
        t = v.Tally(ctx, N_MSG + 2)
        assert t.add_blobs(w.ct_blobs)[1] == 6
        t.result()
        t.free()
    returns_to_baseline(ctx, cycle)


def test_a_context_returns_to_its_baseline(ctx, w):
    """one small call of every family through a fresh context; the handles are made on the shared context before the first reading"""
    cs = w.r1cs(ctx)
    kp = v.Keypair(ctx, cs, w.tox)
    b1, b2 = ctx.upload_bases(w.g1[:64], 1), ctx.upload_bases(w.g2[:64], 2)
    d_scalars = ctx.to_device(w.scalars[:64])
    d_records = ctx.to_device(np.stack([b1.msm_jacobian(d_scalars), b1.msm_jacobian(d_scalars)]))
    spk = v.SaverPublicKey(ctx, w.pk_w, w.gabc[:N_MSG + 1], N_MSG)
    spk.upload()
    rr = v.SaverRerandomizer(ctx, spk, w.delta_g2)
    ver = w.verifier(ctx)
    ped = v.Pedersen(ctx, w.gens)
    tally = v.Tally(ctx, N_MSG + 2)
    msgs = np.ascontiguousarray(w.W[:, :N_MSG])
    a16 = rand_fr_array(16, 50)
    try:
        def cycle():
            c1 = v.Context(0)
            v.multiexp(c1, w.g1[:64], w.scalars[:64], 1)
            c1.check(c1.lib.vsp_msm_launch(c1.h, 1, b2.h, 0, 64, C.c_void_p(d_scalars)))       # launched, never finished
            dom = v.EvaluationDomain(c1, 16)
            dom.fft(a16)
            dom.free()
            v.groth16_prove_batch(c1, cs, kp.pk, w.W, w.rnd[1], w.rnd[2])
            ct, abc, _, _ = v.saver_encrypt_batch(c1, spk, cs, kp.pk, msgs, w.W, *w.rnd)
            assert not v.saver_rerandomize_batch(c1, rr, rand_fr_array(6, 51).reshape(2, 3, 4) | np.uint64(1), ct, abc)[4].any()
            v.saver_receive_blobs(c1, ver, w.ct_blobs[:2], w.pr_blobs[:2], w.in_blobs[:2], tally=tally)
            v.pedersen_hash_batch(c1, ped, w.sks[:2], 255)
            v.fold_jacobian_device(c1, d_records, 2)
            c1.close()
        returns_to_baseline(ctx, cycle)
    finally:
        tally.free(); ped.free(); ver.free(); rr.free(); spk.free(); ctx.dfree(d_records); ctx.dfree(d_scalars); b2.free(); b1.free(); kp.free(); cs.free()


def test_creates_that_fail_after_their_first_allocation_leave_nothing(ctx, w):
    # matrix B names a column that does not exist; A is valid and its six buffers exist when the check refuses B
    (rpa, cia, coa), (rpb, cib, cob), c = w.csr
    bad = cib.copy(); bad[0] = w.cs.num_vars + 1
    fails_clean(ctx, lambda: v.R1CS(ctx, NC, NI, w.cs.num_vars, (rpa, cia, coa), (rpb, bad, cob), c), "r1cs_upload: column out of range")
    # one point off the curve: x of one point with y of another
    pts = w.g1.copy(); pts[11, 6:] = w.g1[12, 6:]
    fails_clean(ctx, lambda: ctx.upload_bases(pts, 1), "bases: a point is not on the curve")
    # a key blob cut short, and one whose first point record carries the compression flag
    cs = w.r1cs(ctx)
    kp = v.Keypair(ctx, cs, w.tox)
    blob = kp.to_blob()
    kp.free(); cs.free()
    fails_clean(ctx, lambda: v.Keypair.from_blob(ctx, blob[:-1]), "pk_from_blob: a count exceeds the blob")
    flagged = bytearray(blob); flagged[96 + 96 + 192 + 96 + 192 + 8] |= 0x80
    fails_clean(ctx, lambda: v.Keypair.from_blob(ctx, bytes(flagged)),
                "pk_from_blob: a point record is not a well-formed uncompressed record (compressed form, stray flag bits, or an infinity record with a payload)")


def test_the_driver_sees_tables_and_replaced_bases_go(ctx, cref):
    """eight cycles of upload 2^15 G1 bases -> window multiples (the 50 MB table replaces the 3 MB of points) -> one multi-exponentiation
    -> free: the device's free memory after the eighth is within 8 MiB of its value after the first.  A leaked table would be 350 MB,
    leaked points 21 MB"""
    hip = C.CDLL("libamdhip64.so")

    def free_bytes():
        f, t = C.c_size_t(0), C.c_size_t(0)
        assert hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
        return f.value
    n = 1 << 15
    pts, scalars = cref.g1_batch_mul_gen(rand_fr_array(n, 60)), rand_fr_array(n, 61)
    d_scalars = ctx.to_device(scalars)
    seen, results = [], []
    try:
        for _ in range(8):
            b = ctx.upload_bases(pts, 1)
            b.precompute(window_bits=16)
            results.append(b.msm(d_scalars)[0].tolist())
            b.free()
            seen.append(free_bytes())
    finally:
        ctx.dfree(d_scalars)
    assert all(r == results[0] for r in results)
    assert abs(seen[7] - seen[0]) < (8 << 20), seen
