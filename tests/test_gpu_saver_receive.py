"""GPU: vsp_saver_receive_blobs on elections of known logs (tests/dlog_election.py: msg_size 2 with one rest input, msg_size 1 with
none).  The blobs are made with the host wire helpers.  The oracle is the composition the call is defined by, computed here from calls
that exist without it, on the same context: Tally.add_blobs (ciphertext status bytes, expected tally), proofs_from_blob_batch (proof
status bytes and limbs), fr_vector_from_blob (input blobs), g1_decompress_batch (member limbs), and saver_verify_batch /
saver_verify_batch_screened on those limbs with every wire-rejected ballot replaced at its own index by a malformed one (A.x = p)."""
import numpy as np
import pytest

import bls12_381 as o

import dlog_election as de

import vote_saver_protocol_amd as v

pytestmark = pytest.mark.gpu
R = o.R
M64 = (1 << 64) - 1
P_LIMBS = [(o.P >> (64 * i)) & M64 for i in range(6)]
KEYS = ("ct", "rest", "A", "B", "C")
DEFAULTS = dict(saver_screen_split=4, saver_screen_chunk=1 << 16, pairing_chunk=1 << 14, tally_chunk_points=1 << 21)
SCREEN_STATS = ("checks", "failed", "exact_ballots")
MODES = ["exact", "screened"]


def coeff_words(zs):
    return np.array([[z & M64, z >> 64] for z in zs], np.uint64).reshape(len(zs), 2)


def random_coeffs(rng, n):
    zs = [rng.randrange(1, 1 << 128) for _ in range(n)]
    zs[0] = 1
    zs[-1] = (1 << 128) - 1
    return zs


def valid_ballot(el, rng, **kw):
    return de.make_ballot(el, [de.nonzero(rng) for _ in range(el.n + 1)], [rng.randrange(R) for _ in range(el.n_rest)], rng, **kw)


class Blobs:
    """the three blobs of every ballot of a batch of limbs, as lists"""

    def __init__(self, el, b):
        n = len(b["A"])
        self.ct = [v.g1_vector_to_blob(b["ct"][k]) for k in range(n)]
        self.pr = [v.g1_compress(b["A"][k]) + v.g2_compress(b["B"][k]) + v.g1_compress(b["C"][k]) for k in range(n)]
        self.inp = [v.fr_vector_to_blob(b["rest"][k]) for k in range(n)] if el.n_rest else None

    def cut(self, sl):
        out = object.__new__(Blobs)
        out.ct, out.pr, out.inp = self.ct[sl], self.pr[sl], None if self.inp is None else self.inp[sl]
        return out

    def patched(self, at, other, k=0):
        """a copy with ballot `at` replaced by ballot k of `other`"""
        out = self.cut(slice(None))
        out.ct[at], out.pr[at] = other.ct[k], other.pr[k]
        if out.inp is not None:
            out.inp[at] = other.inp[k]
        return out

    def __len__(self):
        return len(self.ct)


class Case:
    """an election, its verifier, N valid ballots as blobs, and one ballot of each failing reason to patch in"""

    def __init__(self, ctx, seed, n, n_rest, count):
        self.rng = de.rng(seed)
        self.el = de.Election(self.rng, n, n_rest)
        k = self.el.key
        self.ver = v.SaverVerifier(ctx, self.el.pk_words, k.alpha, k.beta, k.gamma, k.delta, k.gamma_abc, n)
        batch = de.ballot_batch(self.el, [valid_ballot(self.el, self.rng) for _ in range(count)])
        assert batch["want"] == [0] * count
        self.valid = Blobs(self.el, batch)
        self.bad = {}
        for p, z in ((1, 0), (0, 1), (1, 1)):
            one = de.ballot_batch(self.el, [valid_ballot(self.el, self.rng, bump_psi=p, bump_z=z)])
            assert one["want"] == [2 * p + 4 * z]
            self.bad[2 * p + 4 * z] = Blobs(self.el, one)


@pytest.fixture(scope="module")
def cases(ctx, cref):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(ctx, *dict(small=(800, 2, 1, 130), wide=(801, 1, 0, 256))[name])
        return made[name]
    yield get
    for c in made.values():
        c.ver.free()


class options:
    def __init__(self, ctx, **kw):
        self.ctx, self.kw = ctx, kw

    def __enter__(self):
        for k, val in self.kw.items():
            self.ctx.set_option(k, val)

    def __exit__(self, *exc):
        for k in self.kw:
            self.ctx.set_option(k, DEFAULTS[k])


def screen_stats(ctx):
    return {k: int(ctx.stat("saver_screen_" + k)) for k in SCREEN_STATS}


def tally_of(ctx, ct_len, *blob_lists):
    """vsp_tally_result after add_blobs of each list in turn"""
    t = v.Tally(ctx, ct_len)
    try:
        for blobs in blob_lists:
            if len(blobs):
                status, accepted = t.add_blobs(blobs)
                assert accepted == len(blobs) and not status.any()
        ct, ballots = t.result()
    finally:
        t.free()
    return ct, ballots


def composition(ctx, c, b, zs=None, check=True, prior=()):
    """the meaning of the call from the calls that define it -> dict(verdict, reason, wire, stats, tally)"""
    el, N = c.el, len(b)
    t = v.Tally(ctx, el.n + 2)
    try:
        w0, _ = t.add_blobs(b.ct, check_subgroup=check)
    finally:
        t.free()
    A, B, Cc, w1 = v.proofs_from_blob_batch(ctx, b"".join(b.pr), check_subgroup=check)
    rest = np.zeros((N, max(el.n_rest, 1), 4), np.uint64)
    w2 = np.zeros(N, np.uint8)
    for k in range(N if b.inp is not None else 0):
        try:
            vals = v.fr_vector_from_blob(b.inp[k])
            ok = vals.shape[0] == el.n_rest
        except ValueError:
            ok = False
        if ok and el.n_rest:
            rest[k] = vals
        w2[k] = 0 if ok else 1
    pts, _ = v.g1_decompress_batch(ctx, b"".join(blob[8:] for blob in b.ct), check_subgroup=check)
    ct = pts.reshape(N, el.n + 2, 12)
    wire = np.stack([w0, w1, w2], axis=1)
    rejected = wire.any(axis=1)
    A = A.copy()
    A[rejected] = 0
    A[rejected, :6] = P_LIMBS                                        # a malformed ballot at the same index
    ctx.stats_reset()
    if zs is None:
        verdict, reason = v.saver_verify_batch(ctx, c.ver, ct, rest if el.n_rest else None, A, B, Cc)
    else:
        verdict, reason = v.saver_verify_batch_screened(ctx, c.ver, ct, rest if el.n_rest else None, A, B, Cc, coeff_words(zs))
    stats = screen_stats(ctx)
    assert all(reason[k] == 1 and verdict[k] == 0 for k in range(N) if rejected[k])
    tally = tally_of(ctx, el.n + 2, list(prior), [b.ct[k] for k in range(N) if verdict[k]])
    return dict(verdict=verdict.tolist(), reason=reason.tolist(), wire=wire.tolist(), stats=stats, tally=tally, accepted=int(verdict.sum()))


def receive(ctx, c, b, zs=None, check=True, prior=(), with_tally=True):
    """the call under test on a fresh tally (after add_blobs of `prior`) -> the same dict"""
    t = v.Tally(ctx, c.el.n + 2) if with_tally else None
    try:
        if with_tally and len(prior):
            t.add_blobs(list(prior))
        ctx.stats_reset()
        verdict, reason, wire, accepted = v.saver_receive_blobs(ctx, c.ver, b.ct, b.pr, b.inp, coeff=None if zs is None else coeff_words(zs), tally=t,
                                                                check_subgroup=check)
        stats = screen_stats(ctx)
        assert int(ctx.stat("saver_receive_ballots")) == len(b) and int(ctx.stat("saver_receive_wire_rejected")) == int(wire.any(axis=1).sum())
        assert ctx.stat("saver_receive_prepare_ms") > 0
        tally = t.result() if with_tally else None
    finally:
        if t is not None:
            t.free()
    assert verdict.tolist() == [int(r == 0) for r in reason]
    return dict(verdict=verdict.tolist(), reason=reason.tolist(), wire=wire.tolist(), stats=stats, tally=tally, accepted=accepted)


def same(got, want, stats=True):
    assert got["verdict"] == want["verdict"] and got["reason"] == want["reason"] and got["wire"] == want["wire"]
    assert got["accepted"] == want["accepted"]
    if got["tally"] is not None:
        assert np.array_equal(got["tally"][0], want["tally"][0]) and got["tally"][1] == want["tally"][1]
    if stats:
        assert got["stats"] == want["stats"]


def coeffs_for(mode, seed, n):
    return random_coeffs(de.rng(seed), n) if mode == "screened" else None


# 1
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130])
def test_all_valid_ballots_are_accepted_and_tallied(ctx, cases, n, mode):
    c = cases("small")
    b = c.valid.cut(slice(130 - n, 130))
    got = receive(ctx, c, b, coeffs_for(mode, 810 + n, n))
    assert got["reason"] == [0] * n and got["accepted"] == n and not np.array(got["wire"]).any()
    want_ct, want_ballots = tally_of(ctx, c.el.n + 2, b.ct)
    assert np.array_equal(got["tally"][0], want_ct) and got["tally"][1] == want_ballots == n and want_ct.any()
    assert got["stats"] == (dict(checks=1, failed=0, exact_ballots=0) if mode == "screened" else dict(checks=0, failed=0, exact_ballots=0))


# 2
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("at", [0, 128, 255])
@pytest.mark.parametrize("reason", [2, 4, 6])
def test_one_bad_ballot_gets_the_compositions_verdict_and_stays_out_of_the_tally(ctx, cases, reason, at, mode):
    c = cases("wide")
    b = c.valid.patched(at, c.bad[reason])
    zs = coeffs_for(mode, 820 + at + reason, 256)
    want = composition(ctx, c, b, zs)
    assert want["reason"] == [reason if k == at else 0 for k in range(256)]
    got = receive(ctx, c, b, zs)
    same(got, want)                                                  # default piece options: the three saver_screen_* counters too
    others = tally_of(ctx, c.el.n + 2, [b.ct[k] for k in range(256) if k != at])
    assert np.array_equal(got["tally"][0], others[0]) and got["tally"][1] == 255
    if mode == "screened":
        assert got["stats"]["checks"] == 5 and got["stats"]["failed"] == 2 and 1 <= got["stats"]["exact_ballots"] <= 64


# 3
def bad_encodings():
    """the shapes of tests/test_gpu_tally.py bad_encodings(): name -> (48 bytes of a G1 record, status with the subgroup check, without)"""
    x_is_p = bytearray(o.P.to_bytes(48, "big")); x_is_p[0] |= 0x80
    xn = next(x for x in range(5, 200) if o.fp_sqrt((x ** 3 + 4) % o.P) is None)
    non_residue = bytearray(xn.to_bytes(48, "big")); non_residue[0] |= 0x80
    four = bytearray((4).to_bytes(48, "big")); four[0] |= 0x80
    y4 = o.fp_sqrt(68)
    assert y4 is not None and o.G1.is_on_curve((4, y4)) and not o.G1.in_subgroup((4, y4))
    return {"x_equals_p": (bytes(x_is_p), 1, 1), "not_on_curve": (bytes(non_residue), 2, 2), "outside_subgroup": (bytes(four), 4, 0)}


def with_member(blob, j, record):
    return blob[:8 + 48 * j] + record + blob[8 + 48 * (j + 1):]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("check", [True, False])
def test_each_wire_rejection_in_one_ballot_among_good_ones(ctx, cases, check, mode):
    c = cases("small")
    enc = bad_encodings()
    b = c.valid.cut(slice(0, 70))
    want_wire = {}                                                   # ballot -> (byte index, value)
    b.ct[0] = with_member(b.ct[0], 1, enc["x_equals_p"][0]); want_wire[0] = (0, 1)
    b.ct[17] = with_member(b.ct[17], 3, enc["not_on_curve"][0]); want_wire[17] = (0, 2)                   # psi
    b.ct[63] = with_member(b.ct[63], 0, enc["outside_subgroup"][0]); want_wire[63] = (0, 4 if check else 0)
    b.ct[64] = (3).to_bytes(8, "big") + b.ct[64][8:]; want_wire[64] = (0, 1)                              # a wrong count header
    b.pr[65] = enc["x_equals_p"][0] + b.pr[65][48:]; want_wire[65] = (1, 0x11)                            # A
    clear = bytearray(b.pr[20]); clear[48] &= 0x7F                                                        # B without its compression flag
    b.pr[20] = bytes(clear); want_wire[20] = (1, 0x21)
    b.pr[40] = b.pr[40][:144] + enc["not_on_curve"][0]; want_wire[40] = (1, 0x42)                         # C
    b.inp[30] = (1).to_bytes(8, "big") + R.to_bytes(32, "big"); want_wire[30] = (2, 1)                    # a scalar equal to r
    b.inp[50] = (2).to_bytes(8, "big") + b.inp[50][8:]; want_wire[50] = (2, 1)                            # a wrong count
    zs = coeffs_for(mode, 830 + check, 70)
    want = composition(ctx, c, b, zs, check=check)
    got = receive(ctx, c, b, zs, check=check)
    same(got, want)
    for k in range(70):
        triple = [0, 0, 0]
        if k in want_wire:
            triple[want_wire[k][0]] = want_wire[k][1]
        assert got["wire"][k] == triple, k
        if any(triple):
            assert got["reason"][k] == 1 and got["verdict"][k] == 0
        elif k != 63:
            assert got["reason"][k] == 0, k                          # the neighbours in the same wave are unaffected
    if check:
        assert got["reason"][63] == 1 and got["accepted"] == 70 - 9
        if mode == "screened":
            assert got["stats"] == dict(checks=1, failed=0, exact_ballots=0)      # no range fails because of them
    else:
        assert got["reason"][63] not in (0, 1)                       # a curve point of another order in c_0: an equation fails
    accepted = [b.ct[k] for k in range(70) if got["verdict"][k]]
    sums = tally_of(ctx, c.el.n + 2, accepted)
    assert np.array_equal(got["tally"][0], sums[0]) and got["tally"][1] == len(accepted)


def test_header_only_input_blobs_where_there_are_no_rest_inputs(ctx, cases):
    c = cases("wide")
    b = c.valid.cut(slice(0, 5))
    b.inp = [bytes(8)] * 5
    b.inp[3] = (1).to_bytes(8, "big")
    got = receive(ctx, c, b, random_coeffs(de.rng(835), 5))
    assert got["wire"] == [[0, 0, int(k == 3)] for k in range(5)] and got["reason"] == [int(k == 3) for k in range(5)]
    assert got["stats"] == dict(checks=1, failed=0, exact_ballots=0) and got["tally"][1] == 4


# 4
@pytest.mark.parametrize("which,reason", [("bump_psi", 2), ("bump_z", 4)])
def test_the_cancelling_pair_goes_by_original_index(ctx, cases, which, reason):
    """ballots 1 and 3 of five carry the defects z_3 and -z_1: accepted together under (.., z_1, .., z_3, ..) exactly as
    saver_verify_batch_screened accepts them, rejected under the swapped coefficients.  Ballot 2 is wire-rejected: a call that
    compacted the well-formed ballots would pair the coefficients with other ballots"""
    c = cases("small")
    rng = de.rng(840 + reason)
    zs = [rng.randrange(1, 1 << 128) for _ in range(5)]
    pair = Blobs(c.el, de.ballot_batch(c.el, [valid_ballot(c.el, rng, **{which: zs[3]}), valid_ballot(c.el, rng, **{which: R - zs[1]})]))
    b = c.valid.cut(slice(0, 5)).patched(1, pair, 0).patched(3, pair, 1)
    b.ct[2] = (0).to_bytes(8, "big") + b.ct[2][8:]
    want = composition(ctx, c, b, zs)
    assert want["reason"] == [0, 0, 1, 0, 0] and want["stats"] == dict(checks=1, failed=0, exact_ballots=0)
    same(receive(ctx, c, b, zs), want)
    zs[1], zs[3] = zs[3], zs[1]
    want = composition(ctx, c, b, zs)
    assert want["reason"] == [0, reason, 1, reason, 0]
    same(receive(ctx, c, b, zs), want)
    same(receive(ctx, c, b, None), composition(ctx, c, b, None))


# 5
@pytest.mark.parametrize("mode,opts", [("screened", dict(saver_screen_chunk=32)), ("exact", dict(pairing_chunk=32)), ("screened", dict(tally_chunk_points=100)),
                                       ("exact", dict(tally_chunk_points=100))])
def test_pieces_give_the_verdicts_and_the_tally_of_one_piece(ctx, cases, mode, opts):
    """130 ballots in pieces of 32 (or of 100 / 4 = 25 points' worth); ballots 40 and 70 are bad, 100 is wire-rejected: with pieces of 32
    the failing sub-range of ballot 40 lies in the second piece and reaches the exact path from the decoded points"""
    c = cases("small")
    b = c.valid.patched(40, c.bad[4]).patched(70, c.bad[2])
    b.pr[100] = b.pr[100][:144] + bad_encodings()["x_equals_p"][0]
    zs = coeffs_for(mode, 850, 130)
    want = composition(ctx, c, b, zs)
    assert want["reason"] == [{40: 4, 70: 2, 100: 1}.get(k, 0) for k in range(130)]
    one = receive(ctx, c, b, zs)
    same(one, want)
    with options(ctx, **opts):
        got = receive(ctx, c, b, zs)
    same(got, want, stats=False)
    if mode == "screened":
        pieces = 5 if "saver_screen_chunk" in opts else 6
        assert got["stats"]["checks"] == pieces + 2 * 4 and got["stats"]["failed"] == 4 and 2 <= got["stats"]["exact_ballots"] <= 16


# 6
def test_tally_semantics(ctx, cases):
    c = cases("small")
    rng = de.rng(860)
    zs = random_coeffs(rng, 130)
    # the same valid ballot five times
    five = c.valid.cut(slice(7, 8))
    five.ct, five.pr, five.inp = five.ct * 5, five.pr * 5, five.inp * 5
    for z in (zs[:5], None):
        got = receive(ctx, c, five, z)
        assert got["reason"] == [0] * 5
        same(got, composition(ctx, c, five, z))
    # a running tally that already holds ballots from add_blobs
    prior = c.valid.ct[100:130]
    b = c.valid.cut(slice(0, 66)).patched(9, c.bad[6])
    got = receive(ctx, c, b, zs[:66], prior=prior)
    same(got, composition(ctx, c, b, zs[:66], prior=prior))
    assert got["tally"][1] == 30 + 65
    # no tally: verdicts only
    alone = receive(ctx, c, b, zs[:66], with_tally=False)
    assert alone["tally"] is None and alone["reason"] == got["reason"] and alone["accepted"] == 65
    # two calls against one call
    t = v.Tally(ctx, c.el.n + 2)
    try:
        halves = (b.cut(slice(0, 33)), b.cut(slice(33, 66)))
        acc = [v.saver_receive_blobs(ctx, c.ver, h.ct, h.pr, h.inp, coeff=coeff_words(z), tally=t)[3] for h, z in zip(halves, (zs[:33], zs[33:66]))]
        assert acc == [32, 33]
        two = t.result()
    finally:
        t.free()
    one = receive(ctx, c, b, zs[:66])
    assert np.array_equal(two[0], one["tally"][0]) and two[1] == one["tally"][1] == 65


def test_accepted_ballots_with_infinity_members_and_sums_through_infinity(ctx, cases):
    c = cases("small")
    el, rng = c.el, de.rng(870)
    xs = lambda: [rng.randrange(R) for _ in range(el.n_rest)]
    ms = []
    for i in range(12):
        us = [de.nonzero(rng) for _ in range(el.n + 1)]
        if i % 3 == 0: us[i % (el.n + 1)] = 0                       # a member at infinity
        if i == 5: us = [0] * (el.n + 1)                            # every member, psi too
        ms.append(de.make_ballot(el, us, xs(), rng))
    ms += [de.make_ballot(el, [R - u for u in ms[1]["us"]], xs(), rng)]      # ballot 12 = -ballot 1 in every ciphertext member
    batch = de.ballot_batch(el, ms)
    assert batch["want"] == [0] * 13
    b = Blobs(el, batch)
    assert any(blob[8] == 0xC0 for blob in b.ct)                     # an infinity record on the wire
    for z in (random_coeffs(rng, 13), None):
        got = receive(ctx, c, b, z)
        assert got["reason"] == [0] * 13
        same(got, composition(ctx, c, b, z))
    # the running sum passes through infinity: ballots 1 and 12 alone
    pair = b.cut(slice(1, 2)); pair.ct += b.ct[12:]; pair.pr += b.pr[12:]; pair.inp += b.inp[12:]
    got = receive(ctx, c, pair, None)
    assert got["reason"] == [0, 0] and got["tally"][1] == 2 and not got["tally"][0][:el.n + 1].any()


# 7
def test_errors_leave_the_tally_and_the_context_as_they_were(ctx, cases, cref):
    c = cases("small")
    lib, p = ctx.lib, v.api._ptr
    b = c.valid.cut(slice(0, 3))
    ct, pr, inp = (np.frombuffer(b"".join(x), np.uint8) for x in (b.ct, b.pr, b.inp))
    z = coeff_words([5, 6, 7])
    verdict = np.zeros(3, np.uint8)
    t = v.Tally(ctx, c.el.n + 2)
    other = v.Tally(ctx, c.el.n + 3)
    try:
        t.add_blobs(c.valid.ct[10:12])
        before = t.result()
        call = lambda *a: lib.vsp_saver_receive_blobs(*a)
        ERR_ARG = call(None, c.ver.h, t.h, p(ct), p(pr), p(inp), 3, 1, p(z), p(verdict), None, None, None)
        assert ERR_ARG != 0
        ctx.stats_reset()
        for args in ((None, t.h, p(ct), p(pr), p(inp), 3), (c.ver.h, t.h, None, p(pr), p(inp), 3), (c.ver.h, t.h, p(ct), None, p(inp), 3),
                     (c.ver.h, t.h, p(ct), p(pr), None, 3),           # n_rest = 1: the input blobs are required
                     (c.ver.h, other.h, p(ct), p(pr), p(inp), 3),     # a tally of another ct_len
                     (c.ver.h, t.h, None, None, None, 0)):            # also with count = 0
            for coeff in (p(z), None):
                assert call(ctx.h, *args, 1, coeff, p(verdict), None, None, None) == ERR_ARG, args
        assert call(ctx.h, c.ver.h, t.h, p(ct), p(pr), p(inp), 3, 1, p(z), None, None, None, None) == ERR_ARG
        assert call(ctx.h, c.ver.h, t.h, p(ct), p(pr), p(inp), 3, 1, p(coeff_words([5, 0, 7])), p(verdict), None, None, None) == ERR_ARG
        assert "zero" in ctx.last_error()
        # with coefficients, a proof in flight on the context owns the work slots
        cs, wit = cref.R1CS.synth(70, 3, 1)
        dcs = v.R1CS(ctx, 70, 3, cs.num_vars, *cs.export())
        rnd = de._fr([de.nonzero(c.rng) for _ in range(7)])
        kp = v.Keypair(ctx, dcs, rnd[:5])
        try:
            v.groth16_prove_launch(ctx, dcs, kp.pk, wit, rnd[5], rnd[6])
            try:
                assert call(ctx.h, c.ver.h, t.h, p(ct), p(pr), p(inp), 3, 1, p(z), p(verdict), None, None, None) == ERR_ARG
                assert "in flight" in ctx.last_error()
            finally:
                v.groth16_prove_finish(ctx)
        finally:
            kp.free(); dcs.free(); cs.free()
        import torch
        if torch.cuda.device_count() > 1:                           # a verifier of another device
            with v.Context(1) as ctx1:
                k = c.el.key
                ver1 = v.SaverVerifier(ctx1, c.el.pk_words, k.alpha, k.beta, k.gamma, k.delta, k.gamma_abc, c.el.n)
                try:
                    assert call(ctx.h, ver1.h, t.h, p(ct), p(pr), p(inp), 3, 1, p(z), p(verdict), None, None, None) == ERR_ARG
                finally:
                    ver1.free()
        # all of it before any GPU work, and the handle untouched
        assert int(ctx.stat("saver_receive_ballots")) == 0 and int(ctx.stat("saver_screen_checks")) == 0
        after = t.result()
        assert np.array_equal(before[0], after[0]) and before[1] == after[1] == 2
        accepted = np.zeros(1, np.uint64)
        assert call(ctx.h, c.ver.h, t.h, p(ct), p(pr), p(inp), 0, 1, p(z), p(verdict), None, None, p(accepted)) == 0      # no ballots: nothing to do
        assert accepted[0] == 0 and t.result()[1] == 2
        with pytest.raises(ValueError):
            v.saver_receive_blobs(ctx, c.ver, b.ct, b.pr[:2], b.inp)
        with pytest.raises(ValueError):
            v.saver_receive_blobs(ctx, c.ver, b.ct, b.pr, b.inp, coeff=coeff_words([1, 2]))
        # a following valid call gives the right answer
        for coeff in (z, None):
            verdict, reason, wire, acc = v.saver_receive_blobs(ctx, c.ver, b.ct, b.pr, b.inp, coeff=coeff, tally=t)
            assert verdict.tolist() == [1, 1, 1] and not reason.any() and not wire.any() and acc == 3
        want = tally_of(ctx, c.el.n + 2, c.valid.ct[10:12], b.ct, b.ct)
        got = t.result()
        assert np.array_equal(got[0], want[0]) and got[1] == want[1] == 8
    finally:
        t.free(); other.free()
