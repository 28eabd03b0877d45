"""GPU: vsp_saver_verify_batch_screened on elections of known logs (tests/dlog_election.py): the expected reason of every ballot is an
integer congruence, the exact path (vsp_saver_verify_batch) on the same arrays is the second witness, and the statistics say which
ballots were judged by a combined equation and which by the exact path.  Shapes: msg_size 1 and 2, n_rest 0 and 1, N up to 260 around
the 64-lane block edge and the 16-value edge of the product tree, one case of 4097 ballots for the tree's deeper levels.  "saver_screen_split"
is set explicitly in every call (SPLIT unless a test says otherwise)."""
import numpy as np
import pytest

import bls12_381 as o

import dlog_election as de

import vote_saver_protocol_amd as v

pytestmark = pytest.mark.gpu
R = o.R
M64 = (1 << 64) - 1
TOP = (1 << 128) - 1
SPLIT = 4
KEYS = ("ct", "rest", "A", "B", "C")


def coeff_words(zs):
    return np.array([[z & M64, z >> 64] for z in zs], np.uint64).reshape(len(zs), 2)


def random_coeffs(rng, n):
    """n coefficients in [1, 2^128), 1 and 2^128 - 1 among them"""
    zs = [rng.randrange(1, 1 << 128) for _ in range(n)]
    zs[0] = 1
    zs[-1] = TOP
    return zs


def make_verifier(ctx, el):
    k = el.key
    return v.SaverVerifier(ctx, el.pk_words, k.alpha, k.beta, k.gamma, k.delta, k.gamma_abc, el.n)


def valid_ballot(el, rng, **kw):
    return de.make_ballot(el, [de.nonzero(rng) for _ in range(el.n + 1)], [rng.randrange(R) for _ in range(el.n_rest)], rng, **kw)


def cut(b, sl):
    return {k: (None if b[k] is None else b[k][sl]) for k in KEYS} | {"want": b["want"][sl]}


def patched(b, at, single):
    """a copy of the batch with ballot `at` replaced by the one ballot of `single`"""
    out = {k: (None if b[k] is None else b[k].copy()) for k in KEYS}
    for k in KEYS:
        if out[k] is not None:
            out[k][at] = single[k][0]
    out["want"] = list(b["want"]); out["want"][at] = single["want"][0]
    return out


def exact(ctx, ver, b):
    verdict, reason = v.saver_verify_batch(ctx, ver, b["ct"], b["rest"], b["A"], b["B"], b["C"])
    assert verdict.tolist() == [int(r == 0) for r in reason]
    return reason.tolist()


def screened(ctx, ver, b, zs, split=SPLIT, chunk=None):
    """-> (reasons, statistics of the call)"""
    ctx.set_option("saver_screen_split", split)
    if chunk is not None:
        ctx.set_option("saver_screen_chunk", chunk)
    ctx.stats_reset()
    try:
        verdict, reason = v.saver_verify_batch_screened(ctx, ver, b["ct"], b["rest"], b["A"], b["B"], b["C"], coeff_words(zs))
    finally:
        ctx.set_option("saver_screen_split", 4)
        ctx.set_option("saver_screen_chunk", 1 << 16)
    assert verdict.tolist() == [int(r == 0) for r in reason]
    return reason.tolist(), {k: int(ctx.stat("saver_screen_" + k)) for k in ("checks", "failed", "exact_ballots")}


class Case:
    """an election, its verifier and N valid ballots; one ballot of each failing reason to patch in"""

    def __init__(self, ctx, seed, n, n_rest, count):
        self.rng = de.rng(seed)
        self.el = de.Election(self.rng, n, n_rest)
        self.ver = make_verifier(ctx, self.el)
        self.valid = de.ballot_batch(self.el, [valid_ballot(self.el, self.rng) for _ in range(count)])
        assert self.valid["want"] == [0] * count
        self.bad = {2 * p + 4 * z: de.ballot_batch(self.el, [valid_ballot(self.el, self.rng, bump_psi=p, bump_z=z)]) for p, z in ((1, 0), (0, 1), (1, 1))}
        assert [self.bad[r]["want"] for r in (2, 4, 6)] == [[2], [4], [6]]


@pytest.fixture(scope="module")
def cases(ctx, cref):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(ctx, *dict(small=(700, 2, 1, 130), wide=(701, 1, 0, 256))[name])
        return made[name]
    yield get
    for c in made.values():
        c.ver.free()


# 1
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130])
def test_all_valid_ballots_are_accepted_by_one_check(ctx, cases, n):
    c = cases("small")
    reasons, st = screened(ctx, c.ver, cut(c.valid, slice(130 - n, 130)), random_coeffs(de.rng(710 + n), n))
    assert reasons == [0] * n
    assert st == dict(checks=1, failed=0, exact_ballots=0)


# 2
@pytest.mark.parametrize("at", [0, 128, 255])
@pytest.mark.parametrize("reason", [2, 4, 6])
def test_one_bad_ballot_is_found_and_only_its_sub_range_is_judged_exactly(ctx, cases, reason, at):
    c = cases("wide")
    b = patched(c.valid, at, c.bad[reason])
    reasons, st = screened(ctx, c.ver, b, random_coeffs(de.rng(720 + at + reason), 256), split=4)
    assert reasons == b["want"] and reasons[at] == reason and sum(reasons) == reason
    assert reasons == exact(ctx, c.ver, b)
    assert 1 <= st["exact_ballots"] <= 64
    assert st["checks"] == 5 and st["failed"] == 2


# 3
@pytest.mark.parametrize("reason,at,split", [(2, 0, 0), (6, 128, 0), (4, 255, 1)])
def test_without_a_second_level_the_whole_piece_goes_to_the_exact_path(ctx, cases, reason, at, split):
    c = cases("wide")
    b = patched(c.valid, at, c.bad[reason])
    reasons, st = screened(ctx, c.ver, b, random_coeffs(de.rng(730 + at), 256), split=split)
    assert reasons == b["want"] == exact(ctx, c.ver, b)
    assert st == dict(checks=1, failed=1, exact_ballots=256)


# 4
@pytest.mark.parametrize("which,reason", [("bump_psi", 2), ("bump_z", 4)])
def test_coefficients_are_applied_per_ballot(ctx, cases, which, reason):
    """ballots 1 and 3 of five carry the defects z_3 and -z_1: under the coefficients (.., z_1, .., z_3, ..) the defects cancel and both are
    ACCEPTED -- the documented behaviour for coefficients that are not independent of the ballots -- and under the swapped coefficients
    both are rejected by the exact path.  An implementation that ignores coeff, or calls the exact path alone, fails one half"""
    c = cases("small")
    rng = de.rng(740 + reason)
    zs = [rng.randrange(1, 1 << 128) for _ in range(5)]
    pair = de.ballot_batch(c.el, [valid_ballot(c.el, rng, **{which: zs[3]}), valid_ballot(c.el, rng, **{which: R - zs[1]})])
    assert pair["want"] == [reason, reason]
    b = patched(patched(cut(c.valid, slice(0, 5)), 1, cut(pair, slice(0, 1))), 3, cut(pair, slice(1, 2)))
    assert b["want"] == [0, reason, 0, reason, 0] == exact(ctx, c.ver, b)
    reasons, st = screened(ctx, c.ver, b, zs)
    assert reasons == [0] * 5 and st == dict(checks=1, failed=0, exact_ballots=0)
    zs[1], zs[3] = zs[3], zs[1]
    reasons, st = screened(ctx, c.ver, b, zs)
    assert reasons == b["want"] and st["failed"] >= 2 and st["exact_ballots"] >= 2


# 5
def test_malformed_ballots_get_reason_one_and_fail_no_range(ctx, cases):
    c = cases("small")
    b = {k: c.valid[k][:66].copy() for k in KEYS}
    b["rest"][3, 0] = de._fr([int(sum(int(w) << (64 * i) for i, w in enumerate(b["rest"][3, 0]))) + R])[0]      # the same scalar, not reduced
    b["A"][10, :6] = [(o.P >> (64 * i)) & M64 for i in range(6)]     # a coordinate equal to p
    b["ct"][20, 1, 6] ^= np.uint64(1)                               # points off their curves: ct, A, B, C
    b["A"][21, 0] ^= np.uint64(1)
    b["B"][63, 13] ^= np.uint64(1)
    b["C"][64, 7] ^= np.uint64(1)
    b["ct"][65, 3, 0] ^= np.uint64(1)                               # psi
    want = [1 if k in (3, 10, 20, 21, 63, 64, 65) else 0 for k in range(66)]
    assert exact(ctx, c.ver, b) == want
    reasons, st = screened(ctx, c.ver, b, random_coeffs(de.rng(750), 66))
    assert reasons == want
    assert st == dict(checks=1, failed=0, exact_ballots=0)


# 6
def exceptional(case, name):
    """-> (members, coefficients): every member valid"""
    el, rng = case.el, de.rng(760)
    rnd_us = lambda: [de.nonzero(rng) for _ in range(el.n + 1)]
    rnd_xs = lambda: [rng.randrange(R) for _ in range(el.n_rest)]
    z = rng.randrange(1, 1 << 128)
    if name == "copies":                                            # every bucket holds 130 equal points
        m = de.make_ballot(el, rnd_us(), rnd_xs(), rng)
        return [m] * 130, [z] * 130
    if name == "opposite":                                          # u and -u under one coefficient: every bucket cancels, every ciphertext column sums to infinity
        ms = []
        for _ in range(33):
            us = rnd_us()
            ms += [de.make_ballot(el, us, rnd_xs(), rng), de.make_ballot(el, [R - u for u in us], rnd_xs(), rng)]
        return ms, [z] * 66
    if name == "infinity_members":
        ms = []
        for i in range(66):
            us = rnd_us()
            if i % 3 == 0: us[i % (el.n + 1)] = 0
            if i % 11 == 0: us = [0] * (el.n + 1)                   # psi = 0 as well
            ms.append(de.make_ballot(el, us, rnd_xs(), rng))
        return ms, random_coeffs(rng, 66)
    if name == "abc_infinity":
        kws = [dict(s=0), dict(t=0), dict(z=0), {}]
        return [de.make_ballot(el, rnd_us(), rnd_xs(), rng, **kws[i % 4]) for i in range(66)], random_coeffs(rng, 66)
    if name == "column_sum":                                        # column 1: zero but for ballots 5 and 64, z_5 u_5 + z_64 u_64 = 0 under distinct coefficients
        zs = random_coeffs(rng, 66)
        ms = []
        u5 = de.nonzero(rng)
        for i in range(66):
            us = rnd_us()
            us[1] = u5 if i == 5 else ((-zs[5] * u5 * pow(zs[64], -1, R)) % R if i == 64 else 0)
            ms.append(de.make_ballot(el, us, rnd_xs(), rng))
        return ms, zs
    raise KeyError(name)


@pytest.mark.parametrize("name", ["copies", "opposite", "infinity_members", "abc_infinity", "column_sum"])
def test_exceptional_sums_are_exact(ctx, cases, name):
    c = cases("small")
    ms, zs = exceptional(c, name)
    b = de.ballot_batch(c.el, ms)
    assert b["want"] == [0] * len(ms)
    reasons, st = screened(ctx, c.ver, b, zs)
    assert reasons == b["want"] and st == dict(checks=1, failed=0, exact_ballots=0)
    at = len(ms) // 2
    b = patched(b, at, c.bad[6])
    reasons, st = screened(ctx, c.ver, b, zs)
    assert reasons == b["want"] == exact(ctx, c.ver, b) and reasons[at] == 6
    assert 1 <= st["exact_ballots"] <= (len(ms) + SPLIT - 1) // SPLIT and st["failed"] == 2


# 7
def test_pieces_are_judged_on_their_own(ctx, cases):
    c = cases("small")
    b = patched(c.valid, 70, c.bad[4])                              # pieces of 32: ballot 70 is in the third
    reasons, st = screened(ctx, c.ver, b, random_coeffs(de.rng(770), 130), split=4, chunk=32)
    assert reasons == b["want"] == exact(ctx, c.ver, b)
    assert st["checks"] == 5 + 4 and st["failed"] == 2              # five pieces, the third once more in four sub-ranges
    assert 1 <= st["exact_ballots"] <= 32


# 8
def test_deeper_levels_of_the_product_tree(ctx, cref):
    """4097 ballots: levels of 257, 17, 2 and 1 values.  Then ballot 4096, alone in the last lane of every level, bad"""
    rng = de.rng(780)
    el = de.Election(rng, 1, 0)
    ver = make_verifier(ctx, el)
    try:
        b = de.ballot_batch(el, [valid_ballot(el, rng) for _ in range(4097)])
        zs = random_coeffs(rng, 4097)
        reasons, st = screened(ctx, ver, b, zs)
        assert reasons == [0] * 4097 and st == dict(checks=1, failed=0, exact_ballots=0)
        b = patched(b, 4096, de.ballot_batch(el, [valid_ballot(el, rng, bump_z=1)]))
        reasons, st = screened(ctx, ver, b, zs)
        assert reasons == [0] * 4096 + [4]
        assert st["failed"] == 2 and 1 <= st["exact_ballots"] <= 1025
    finally:
        ver.free()


# 9
def test_errors_leave_the_context_usable(ctx, cases):
    c = cases("small")
    lib, p = ctx.lib, v.api._ptr
    b = cut(c.valid, slice(0, 3))
    ct, rest, A, B, Cc = (np.ascontiguousarray(b[k]) for k in KEYS)
    z = coeff_words([5, 6, 7])
    verdict = np.zeros(3, np.uint8)
    call = lambda *a: lib.vsp_saver_verify_batch_screened(*a)
    ERR_ARG = call(None, c.ver.h, p(ct), p(rest), p(A), p(B), p(Cc), 3, p(z), p(verdict), None)
    assert ERR_ARG != 0
    assert call(ctx.h, c.ver.h, p(ct), p(rest), p(A), p(B), p(Cc), 3, None, p(verdict), None) == ERR_ARG            # coeff is required
    assert call(ctx.h, c.ver.h, None, p(rest), p(A), p(B), p(Cc), 3, p(z), p(verdict), None) == ERR_ARG
    assert call(ctx.h, None, p(ct), p(rest), p(A), p(B), p(Cc), 3, p(z), p(verdict), None) == ERR_ARG
    assert call(ctx.h, c.ver.h, p(ct), p(rest), p(A), p(B), p(Cc), 3, p(z), None, None) == ERR_ARG
    assert call(ctx.h, c.ver.h, None, None, None, None, None, 0, None, None, None) == ERR_ARG                    # also with n = 0
    assert call(ctx.h, c.ver.h, p(ct), p(rest), p(A), p(B), p(Cc), 0, p(z), p(verdict), None) == 0                  # no ballots: nothing to do
    ctx.stats_reset()
    assert call(ctx.h, c.ver.h, p(ct), p(rest), p(A), p(B), p(Cc), 3, p(coeff_words([5, 0, 7])), p(verdict), None) == ERR_ARG
    assert "zero" in ctx.last_error() and ctx.stat("saver_screen_checks") == 0                                     # before any GPU work
    with pytest.raises(ValueError):
        v.saver_verify_batch_screened(ctx, c.ver, ct, rest, A, B, Cc, coeff_words([1, 2]))
    import torch
    if torch.cuda.device_count() > 1:                               # a verifier of another device
        with v.Context(1) as other:
            ver1 = make_verifier(other, c.el)
            try:
                assert call(ctx.h, ver1.h, p(ct), p(rest), p(A), p(B), p(Cc), 3, p(z), p(verdict), None) == ERR_ARG
            finally:
                ver1.free()
    assert screened(ctx, c.ver, b, [5, 6, 7]) == ([0, 0, 0], dict(checks=1, failed=0, exact_ballots=0))
    verdict, reason = v.saver_verify_batch_screened(ctx, c.ver, ct, rest, A, B, Cc)          # coefficients drawn from `secrets`
    assert verdict.tolist() == [1, 1, 1] and reason.tolist() == [0, 0, 0]


# 10
@pytest.fixture(scope="module")
def real_election(ctx, cref):
    """ballots of the library's own encrypt and rerandomize, as tests/test_gpu_saver_verify.py builds its module fixture: msg_size 4, three
    real ballots rerandomized four times each"""
    from conftest import I, L, fr_array
    n, nc, ni, seed = 4, 48, 6, 404
    gen = o.splitmix64(seed)
    tox = fr_array([o.rand_fr(gen) for _ in range(5)])
    rnd = fr_array([o.rand_fr(gen) for _ in range(3 * n + 2)])
    dcs = kp = spk = parts = None
    cts, As, Bs, Cs, rests = [], [], [], [], []
    for vote in (0, 3, 1):
        cs, wit = cref.R1CS.synth(nc, ni, seed, ballot=(n, vote))
        if dcs is None:
            dcs = v.R1CS(ctx, nc, ni, cs.num_vars, *cs.export())
            kp = v.Keypair(ctx, dcs, tox)
            parts = {k: kp.part(k) for k in ("gamma_ABC_g1", "delta_g1", "gamma_g1", "alpha_g1", "beta_g2", "gamma_g2", "delta_g2")}
            gabc = np.ascontiguousarray(parts["gamma_ABC_g1"])
            pk_w, _, _ = v.saver_generate_keypair(ctx, rnd, gabc, parts["delta_g1"][0], parts["gamma_g1"][0], n)
            spk = v.SaverPublicKey(ctx, pk_w, gabc[:n + 1], n)
        r_enc, r, s = (L(o.rand_fr(gen), 4) for _ in range(3))
        ct, abc, _ = v.saver_encrypt(ctx, spk, dcs, kp.pk, wit[:n], wit, r_enc, r, s)
        for _ in range(4):
            ct, abc, _ = v.saver_rerandomize(ctx, spk, parts["delta_g2"][0], fr_array([o.rand_fr(gen) for _ in range(3)]), ct, abc)
            cts.append(ct); As.append(abc[0].reshape(12)); Bs.append(abc[1].reshape(24)); Cs.append(abc[2].reshape(12)); rests.append(wit[n:ni].copy())
        cs.free()
    ver = v.SaverVerifier(ctx, pk_w, parts["alpha_g1"][0], parts["beta_g2"][0], parts["gamma_g2"][0], parts["delta_g2"][0], parts["gamma_ABC_g1"], n)
    yield dict(ver=ver, ct=np.stack(cts), rest=np.stack(rests), A=np.stack(As), B=np.stack(Bs), C=np.stack(Cs))
    for h in (ver, spk, kp, dcs):
        h.free()


def test_real_ballots_with_one_tampered_agree_with_the_exact_path(ctx, real_election):
    from conftest import g1_limbs
    e = real_election
    b = {k: e[k].copy() for k in KEYS}
    zs = random_coeffs(de.rng(790), 12)
    assert screened(ctx, e["ver"], b, zs) == ([0] * 12, dict(checks=1, failed=0, exact_ballots=0))
    b["C"][7] = g1_limbs(o.G1.neg(o.g1_from_limbs(b["C"][7])))       # C negated
    want = exact(ctx, e["ver"], b)
    assert want == [4 if k == 7 else 0 for k in range(12)]
    reasons, st = screened(ctx, e["ver"], b, zs)
    assert reasons == want and st["failed"] == 2 and 1 <= st["exact_ballots"] <= 3
