"""GPU: the ballot box (vsp_ballot_box, vsp_ballot_box_receive_blobs) on an election of known logs (tests/dlog_election.py: msg_size 2,
five rest inputs eid | sn_0 | sn_1 | rt | rt2 with the roles FIXED, SERIAL, SERIAL, FIXED, FIXED).  make_ballot takes arbitrary rest
inputs, so valid ballots with chosen eid, serial and roots cost nothing.  The oracle is a Python dict walked in index order: a ballot is
accepted when it is not wire-rejected, its FIXED inputs are the box's, both equations hold (the congruences of dlog_election) and no
earlier accepted ballot holds its serial; the expected tally is Tally.add_blobs over exactly the accepted ballots' ciphertext blobs."""
import ctypes as C

import numpy as np
import pytest

import bls12_381 as o

import dlog_election as de

import vote_saver_protocol_amd as v

pytestmark = pytest.mark.gpu
R = o.R
M64 = (1 << 64) - 1
NONE = (1 << 64) - 1
EID, RT, RT2 = 0x5eed0001, (R - 12345) // 3, 0x77 << 200
ROLES = [v.api.FIXED, v.api.SERIAL, v.api.SERIAL, v.api.FIXED, v.api.FIXED]
DEFAULTS = dict(saver_screen_split=4, saver_screen_chunk=1 << 16, pairing_chunk=1 << 14, tally_chunk_points=1 << 21, ballot_box_table_bits=16)
MODES = ["exact", "screened"]
X_IS_P = bytes([o.P.to_bytes(48, "big")[0] | 0x80]) + o.P.to_bytes(48, "big")[1:]


def coeff_words(zs):
    return np.array([[z & M64, z >> 64] for z in zs], np.uint64).reshape(len(zs), 2)


def coeffs_for(mode, seed, n):
    if mode != "screened":
        return None
    rng = de.rng(seed)
    return [rng.randrange(1, 1 << 128) for _ in range(n)]


class Rec:
    """one ballot: its three blobs and what the model needs to know of it"""

    def __init__(self, ct, pr, inp, serial, fixed, vreason, wire=False):
        self.ct, self.pr, self.inp, self.serial, self.fixed, self.vreason, self.wire = ct, pr, inp, serial, fixed, vreason, wire

    def wire_rejected(self):
        """the same ballot with A's x = p on the wire"""
        return Rec(self.ct, X_IS_P + self.pr[48:], self.inp, self.serial, self.fixed, self.vreason, True)


class World:
    def __init__(self, ctx, seed=900, n=2, n_rest=5, pool=130):
        self.ctx, self.rng = ctx, de.rng(seed)
        self.el = de.Election(self.rng, n, n_rest)
        k = self.el.key
        self.ver = v.SaverVerifier(ctx, self.el.pk_words, k.alpha, k.beta, k.gamma, k.delta, k.gamma_abc, n)
        self.expected = de._fr([EID, 0, 0, RT, RT2])
        self.pool = self.make([dict(sn=(1000 + i, 7)) for i in range(pool)]) if pool else []

    def make(self, specs):
        """specs: dict(sn=(a, b), eid=, rt=, rt2=, bump_psi=, bump_z=) per ballot -> [Rec]"""
        el, members, fixed = self.el, [], []
        for s in specs:
            xs = [s.get("eid", EID), s["sn"][0], s["sn"][1], s.get("rt", RT), s.get("rt2", RT2)]
            fixed.append((xs[0], xs[3], xs[4]) == (EID, RT, RT2))
            members.append(de.make_ballot(el, [de.nonzero(self.rng) for _ in range(el.n + 1)], xs, self.rng, bump_psi=s.get("bump_psi", 0), bump_z=s.get("bump_z", 0)))
        b = de.ballot_batch(el, members)
        return [Rec(v.g1_vector_to_blob(b["ct"][k]), v.g1_compress(b["A"][k]) + v.g2_compress(b["B"][k]) + v.g1_compress(b["C"][k]), v.fr_vector_to_blob(b["rest"][k]),
                    tuple(specs[k]["sn"]), fixed[k], b["want"][k]) for k in range(len(specs))]

    def box(self, roles=ROLES):
        return v.BallotBox(self.ctx, self.ver, self.expected, roles)

    def free(self):
        self.ver.free()


@pytest.fixture(scope="module")
def w(ctx, cref):
    world = World(ctx)
    yield world
    world.free()


class options:
    def __init__(self, ctx, **kw):
        self.ctx, self.kw = ctx, kw

    def __enter__(self):
        for k, val in self.kw.items():
            self.ctx.set_option(k, val)

    def __exit__(self, *exc):
        for k in self.kw:
            self.ctx.set_option(k, DEFAULTS[k])


def tally_of(ctx, ct_len, blobs):
    t = v.Tally(ctx, ct_len)
    try:
        if len(blobs):
            status, accepted = t.add_blobs(blobs)
            assert accepted == len(blobs) and not status.any()
        return t.result()
    finally:
        t.free()


def serial_rows(serials):
    """[(a, b)] -> [n, 2, 4] canonical scalars, as BallotBox.serials exports them"""
    return de._fr([x for s in serials for x in s]).reshape(len(serials), 2, 4)


def model(state, recs):
    """walks recs in index order over state (the accepted serials in ordinal order; extended in place) -> (verdict, reasons, holder):
    reasons[k] is the set a conforming call may give -- two members only where the ballot both fails an equation and repeats a serial"""
    held = {s: i for i, s in enumerate(state)}
    verdict, reasons, holder = [], [], []
    for r in recs:
        ok, why, by = 0, None, NONE
        if r.wire:
            why = {1}
        elif not r.fixed:
            why = {8}
        elif r.serial in held:
            why, by = ({16, r.vreason} if r.vreason else {16}), held[r.serial]
        elif r.vreason:
            why = {r.vreason}
        else:
            ok, why = 1, {0}
            held[r.serial] = len(state)
            state.append(r.serial)
        verdict.append(ok); reasons.append(why); holder.append(by)
    return verdict, reasons, holder


def receive(box, recs, zs=None, tally=None):
    verdict, reason, wire, accepted, holder = box.receive_blobs([r.ct for r in recs], [r.pr for r in recs], [r.inp for r in recs],
                                                                coeff=None if zs is None else coeff_words(zs), tally=tally)
    assert accepted == int(verdict.sum())
    return dict(verdict=verdict.tolist(), reason=reason.tolist(), wire=wire.tolist(), holder=[int(h) for h in holder])


def run(w, recs, mode, seed, cuts=(), roles=ROLES, prior=()):
    """a fresh box (prior: serials added first) and a fresh tally; recs in len(cuts) + 1 calls -> the outputs joined, the tally, the export"""
    ctx = w.ctx
    box, t = w.box(roles), v.Tally(ctx, w.el.n + 2)
    try:
        if len(prior):
            status, added = box.add_serials(serial_rows(prior))
            assert added == len(prior) and not status.any()
        zs = coeffs_for(mode, seed, len(recs))
        out = dict(verdict=[], reason=[], wire=[], holder=[])
        edges = [0] + list(cuts) + [len(recs)]
        for lo, hi in zip(edges[:-1], edges[1:]):
            got = receive(box, recs[lo:hi], None if zs is None else zs[lo:hi], t)
            for key in out:
                out[key] += got[key]
        out["tally"] = t.result()
        out["count"] = box.count()
        out["serials"] = box.serials()
        return out
    finally:
        box.free(); t.free()


def check(w, got, recs, prior=()):
    """the outputs against the model and the tally against Tally.add_blobs of the accepted ballots"""
    state = list(prior)
    verdict, reasons, holder = model(state, recs)
    assert got["verdict"] == verdict
    assert all(r in why for r, why in zip(got["reason"], reasons)), [(k, r, why) for k, (r, why) in enumerate(zip(got["reason"], reasons)) if r not in why]
    assert got["holder"] == holder
    assert got["wire"] == [[0, 0x11 if r.wire else 0, 0] for r in recs]
    assert got["count"] == len(state) and np.array_equal(got["serials"], serial_rows(state))
    want = tally_of(w.ctx, w.el.n + 2, [r.ct for r, ok in zip(recs, verdict) if ok])
    assert np.array_equal(got["tally"][0], want[0]) and got["tally"][1] == want[1] == sum(verdict)
    return verdict, reasons, holder


# 1
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130])
def test_distinct_valid_ballots_are_what_the_plain_call_makes_of_them(w, n, mode):
    ctx, recs = w.ctx, w.pool[130 - n:]
    zs = coeffs_for(mode, 910 + n, n)
    t = v.Tally(ctx, w.el.n + 2)
    try:
        verdict, reason, wire, accepted = v.saver_receive_blobs(ctx, w.ver, [r.ct for r in recs], [r.pr for r in recs], [r.inp for r in recs],
                                                                coeff=None if zs is None else coeff_words(zs), tally=t)
        plain = t.result()
    finally:
        t.free()
    got = run(w, recs, mode, 910 + n)
    assert got["verdict"] == verdict.tolist() == [1] * n and got["reason"] == reason.tolist() == [0] * n and got["wire"] == wire.tolist()
    assert np.array_equal(got["tally"][0], plain[0]) and got["tally"][1] == plain[1] == n and plain[0].any()
    assert got["holder"] == [NONE] * n
    assert np.array_equal(got["serials"], serial_rows([r.serial for r in recs]))      # index order
    check(w, got, recs)


# 2
@pytest.mark.parametrize("mode", MODES)
def test_a_batch_sent_twice_is_all_spent_and_reaches_no_pairing(w, mode):
    ctx, recs, n = w.ctx, w.pool[:70], 70
    box, t = w.box(), v.Tally(ctx, w.el.n + 2)
    try:
        zs = coeffs_for(mode, 920, n)
        first = receive(box, recs, zs, t)
        assert first["verdict"] == [1] * n
        before, serials = t.result(), box.serials()
        ctx.stats_reset()
        again = receive(box, recs, coeffs_for(mode, 921, n), t)
        assert again["verdict"] == [0] * n and again["reason"] == [16] * n and again["holder"] == list(range(n))
        after = t.result()
        assert np.array_equal(before[0], after[0]) and before[1] == after[1] == n
        assert box.count() == n and np.array_equal(box.serials(), serials)
        # no ballot of the second call reached a pairing: neither the screening nor the exact path ran
        for name in ("saver_screen_checks", "saver_screen_miller_ms", "saver_screen_exact_ballots", "saver_verify_miller_ms", "saver_verify_finalexp_ms"):
            assert ctx.stat(name) == 0, name
        assert int(ctx.stat("ballot_box_spent")) == n and int(ctx.stat("ballot_box_mismatched")) == 0 and ctx.stat("ballot_box_ms") > 0
        assert int(ctx.stat("saver_receive_ballots")) == n
    finally:
        box.free(); t.free()


# 3
def with_repeats(w, recs, first, others):
    """recs with fresh valid ballots of recs[first]'s serial at the indices `others`"""
    out = list(recs)
    for at, rec in zip(others, w.make([dict(sn=recs[first].serial) for _ in others])):
        out[at] = rec
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("first,others", [(0, (1,)), (0, (69,)), (63, (64,)), (3, (17, 63, 64, 69))])
def test_duplicates_within_one_piece_the_first_one_wins(w, first, others, mode):
    recs = with_repeats(w, w.pool[:70], first, others)
    got = run(w, recs, mode, 930 + first)
    verdict, reasons, holder = check(w, got, recs)
    assert [k for k in range(70) if not verdict[k]] == list(others)
    assert all(got["reason"][k] == 16 and got["holder"][k] == first for k in others)
    if len(others) == 4:
        # the same call twenty times: the lanes' race for the slot never shows in a byte of the results
        for _ in range(20):
            again = run(w, recs, mode, 930 + first)
            for key in ("verdict", "reason", "wire", "holder", "count"):
                assert again[key] == got[key]
            assert np.array_equal(again["serials"], got["serials"]) and np.array_equal(again["tally"][0], got["tally"][0]) and again["tally"][1] == got["tally"][1]


# 4
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bump,reason", [("bump_psi", 2), ("bump_z", 4)])
def test_an_invalid_first_occurrence_reserves_nothing(w, bump, reason, mode):
    recs = list(w.pool[:10])
    recs[3] = w.make([dict(sn=recs[6].serial, **{bump: 1})])[0]
    assert recs[3].vreason == reason
    got = run(w, recs, mode, 940 + reason)
    check(w, got, recs)
    assert got["verdict"] == [int(k != 3) for k in range(10)] and got["reason"][3] == reason and got["holder"] == [NONE] * 10
    assert np.array_equal(got["serials"], serial_rows([r.serial for k, r in enumerate(recs) if k != 3]))
    # the other order: the valid one holds the serial, and the invalid one's holder names it under the verifier's reason
    recs[3], recs[6] = recs[6], recs[3]
    got = run(w, recs, mode, 941 + reason)
    check(w, got, recs)
    assert got["reason"][6] == reason and got["holder"][6] == 3


# 5
@pytest.mark.parametrize("mode", MODES)
def test_a_wire_rejected_first_occurrence_reserves_nothing(w, mode):
    recs = list(w.pool[:10])
    recs[3] = w.make([dict(sn=recs[6].serial)])[0].wire_rejected()
    got = run(w, recs, mode, 950)
    check(w, got, recs)
    assert got["verdict"] == [int(k != 3) for k in range(10)] and got["reason"][3] == 1 and got["holder"] == [NONE] * 10
    # a wire-rejected ballot whose serial is spent is still wire-rejected, and holds nothing
    got = run(w, recs, mode, 951, prior=[recs[6].serial])
    check(w, got, recs, prior=[recs[6].serial])
    assert got["reason"][3] == 1 and got["reason"][6] == 16 and got["holder"][3] == NONE and got["holder"][6] == 0


# 6
@pytest.mark.parametrize("mode", MODES)
def test_a_wrong_eid_or_rt_is_turned_away_before_the_verifier(w, mode):
    ctx = w.ctx
    recs = list(w.pool[:12])
    recs[2], recs[5], recs[9] = w.make([dict(sn=(2000, 1), eid=EID + 1), dict(sn=(2001, 1), rt=RT - 1, bump_psi=1), dict(sn=(2002, 1), rt2=0)])
    assert [recs[k].vreason for k in (2, 5, 9)] == [0, 2, 0]
    ctx.stats_reset()
    got = run(w, recs, mode, 960)
    if mode == "screened":
        # ballot 5 also fails an equation: it is out of every sum, so no range fails and nothing reaches the exact path
        assert (int(ctx.stat("saver_screen_checks")), int(ctx.stat("saver_screen_failed")), int(ctx.stat("saver_screen_exact_ballots"))) == (1, 0, 0)
    assert int(ctx.stat("ballot_box_mismatched")) == 3
    check(w, got, recs)
    assert [got["reason"][k] for k in (2, 5, 9)] == [8, 8, 8] and sum(got["verdict"]) == 9
    # FREE in place of the FIXED role: eid is not compared, the ballot is accepted; rt free: ballot 5 reaches the verifier
    free_eid = run(w, recs, mode, 961, roles=[v.api.FREE] + ROLES[1:])
    assert free_eid["reason"][2] == 0 and free_eid["verdict"][2] == 1 and free_eid["reason"][5] == 8 and sum(free_eid["verdict"]) == 10
    free_rt = run(w, recs, mode, 962, roles=ROLES[:3] + [v.api.FREE, v.api.FIXED])
    assert free_rt["reason"][5] == 2 and free_rt["reason"][2] == 8 and free_rt["reason"][9] == 8


# 7
@pytest.mark.parametrize("which,reason", [("bump_psi", 2), ("bump_z", 4)])
def test_the_cancelling_pair_goes_by_original_index_around_a_spent_ballot(w, which, reason):
    """ballots 1 and 3 of five carry the defects z_3 and -z_1: accepted together under (.., z_1, .., z_3, ..), rejected under the swapped
    coefficients.  Ballot 2 is spent: a call that compacted the remaining ballots would pair the coefficients with other ballots"""
    rng = de.rng(970 + reason)
    zs = [rng.randrange(1, 1 << 128) for _ in range(5)]
    recs = list(w.pool[:5])
    recs[1], recs[3] = w.make([dict(sn=recs[1].serial, **{which: zs[3]}), dict(sn=recs[3].serial, **{which: R - zs[1]})])
    prior = [recs[2].serial]

    def call(z):
        box = w.box()
        try:
            box.add_serials(serial_rows(prior))
            return receive(box, recs, z)
        finally:
            box.free()
    got = call(zs)
    assert got["reason"] == [0, 0, 16, 0, 0] and got["holder"] == [NONE, NONE, 0, NONE, NONE]
    zs[1], zs[3] = zs[3], zs[1]
    for z in (zs, None):
        got = call(z)
        assert got["reason"] == [0, reason, 16, reason, 0] and got["verdict"] == [1, 0, 0, 0, 1]


# 8
def mixed_batch(w):
    """130 ballots: repeats (adjacent, across the 64 boundary, far apart, threefold), invalid ones, mismatches, a wire rejection, an
    invalid ballot that repeats an accepted serial (after it) and one that precedes the valid ballot of its serial"""
    recs = list(w.pool)
    sn = lambda k: w.pool[k].serial
    new = w.make([dict(sn=sn(4)), dict(sn=sn(63)), dict(sn=sn(10)), dict(sn=sn(10)), dict(sn=sn(10)), dict(sn=sn(20), bump_z=1), dict(sn=sn(41), bump_psi=1),
                  dict(sn=sn(90), bump_psi=1, bump_z=1), dict(sn=(3000, 3), eid=0), dict(sn=sn(7), rt=RT + 1), dict(sn=sn(100))])
    for at, rec in zip((5, 64, 33, 77, 129, 30, 40, 120, 50, 8, 99), new):
        recs[at] = rec
    recs[99] = recs[99].wire_rejected()                              # the first occurrence of serial 100 is wire-rejected: ballot 100 is accepted
    recs[110] = recs[110].wire_rejected()
    return recs


@pytest.mark.parametrize("mode", MODES)
def test_pieces_and_calls_do_not_change_the_outcome(w, mode):
    ctx, recs = w.ctx, mixed_batch(w)
    small = dict(saver_screen_chunk=32) if mode == "screened" else dict(pairing_chunk=32)
    runs = []
    for opts in ({}, small):
        for cuts in ((), (65,), (26, 52, 78, 104)):
            with options(ctx, **opts):
                runs.append(run(w, recs, mode, 980, cuts))
    verdict, reasons, holder = check(w, runs[0], recs)
    assert verdict[30] == 0 and runs[0]["reason"][30] in (4, 16) and holder[30] == 18 and reasons[120] == {16, 6} and reasons[40] == {2}
    for got in runs[1:]:
        check(w, got, recs)
        for key in ("verdict", "wire", "holder", "count"):
            assert got[key] == runs[0][key]
        assert np.array_equal(got["serials"], runs[0]["serials"]) and np.array_equal(got["tally"][0], runs[0]["tally"][0]) and got["tally"][1] == runs[0]["tally"][1]
        assert all(a == b for a, b, why in zip(got["reason"], runs[0]["reason"], reasons) if len(why) == 1)
    # the piece boundary decides between the two reasons of ballot 30 (its holder, ballot 20, is in its piece or in an earlier one)
    assert runs[0]["reason"][30] == 4 and runs[2]["reason"][30] == 16 and runs[3]["reason"][30] == 4


# 9
@pytest.mark.parametrize("mode", MODES)
def test_tiny_tables_chain_wrap_and_grow_to_the_same_outcome(w, mode):
    ctx, recs = w.ctx, mixed_batch(w)
    cuts = (3, 4, 26, 60, 61, 104)
    want = run(w, recs, mode, 990, cuts)
    ctx.stats_reset()
    with options(ctx, ballot_box_table_bits=2):
        got = run(w, recs, mode, 990, cuts)
    assert int(ctx.stat("ballot_box_grown")) >= 3                    # from 4 slots to 256, a few calls at a time
    check(w, got, recs)
    for key in ("verdict", "reason", "wire", "holder", "count"):
        assert got[key] == want[key]
    assert np.array_equal(got["serials"], want["serials"]) and np.array_equal(got["tally"][0], want["tally"][0])


# 10
@pytest.mark.parametrize("mode", MODES)
def test_an_exported_box_restores_with_its_ordinals(w, mode):
    ctx, recs = w.ctx, w.pool[:70]
    a, b = w.box(), None
    try:
        first = receive(a, recs, coeffs_for(mode, 1000, 70))
        assert first["verdict"] == [1] * 70
        exported = a.serials()
        assert exported.shape == (70, 2, 4) and np.array_equal(a.serials(10, 5), exported[10:15])
        with options(ctx, ballot_box_table_bits=3):
            b = w.box()
        status, added = b.add_serials(exported)
        assert added == 70 and not status.any() and b.count() == 70 and np.array_equal(b.serials(), exported)
        assert b.device_bytes() > 0
        again = receive(b, recs[::-1], coeffs_for(mode, 1001, 70))
        assert again["verdict"] == [0] * 70 and again["reason"] == [16] * 70 and again["holder"] == list(range(69, -1, -1))
        # a list with repeats: of the box's own serials, and of new ones inside the list
        new = serial_rows([(5000, 1), (5001, 1), (5000, 1), (1003, 7), (5002, 1), (5001, 1), (5000, 1)])
        status, added = b.add_serials(new)
        assert status.tolist() == [0, 0, 1, 1, 0, 1, 1] and added == 3 and b.count() == 73
        assert np.array_equal(b.serials(70), serial_rows([(5000, 1), (5001, 1), (5002, 1)]))
        status, added = b.add_serials(new[:0])
        assert added == 0 and b.count() == 73
    finally:
        a.free()
        if b is not None:
            b.free()


# 11
def test_errors_leave_the_tally_the_box_and_the_context_as_they_were(w):
    ctx = w.ctx
    lib, p = ctx.lib, v.api._ptr
    ERR_ARG = -1
    expected = np.ascontiguousarray(w.expected)
    role = np.array(ROLES, np.uint8)

    def create(ver, exp, ro, n_rest):
        h = lib.vsp_ballot_box_create(ctx.h, ver, p(exp) if exp is not None else None, p(ro) if ro is not None else None, n_rest)
        if h:
            lib.vsp_ballot_box_free(ctx.h, h)
        return bool(h)
    assert not create(None, expected, role, 5) and not create(w.ver.h, None, role, 5) and not create(w.ver.h, expected, None, 5)
    assert not create(w.ver.h, expected, role, 0) and not create(w.ver.h, expected, role, 4)
    assert not create(w.ver.h, expected, np.array([1, 2, 3, 1, 1], np.uint8), 5) and "role" in ctx.last_error()
    assert not create(w.ver.h, expected, np.array([1, 0, 0, 1, 1], np.uint8), 5) and "SERIAL" in ctx.last_error()
    not_below_r = expected.copy(); not_below_r[3] = de._fr([R])[0]
    assert not create(w.ver.h, not_below_r, role, 5) and "below r" in ctx.last_error()
    not_below_r[3] = expected[3]; not_below_r[1] = de._fr([R])[0]       # not a FIXED input: ignored
    assert create(w.ver.h, not_below_r, role, 5)
    wide = World(ctx, seed=901, n=1, n_rest=9, pool=0)
    try:
        exp9 = np.zeros((9, 4), np.uint64)
        assert not create(wide.ver.h, exp9, np.full(9, 2, np.uint8), 9) and "SERIAL" in ctx.last_error()
        assert create(wide.ver.h, exp9, np.array([2] * 8 + [0], np.uint8), 9)
    finally:
        wide.free()
    recs = w.pool[:3]
    ct, pr, inp = (np.frombuffer(b"".join(x), np.uint8) for x in ([r.ct for r in recs], [r.pr for r in recs], [r.inp for r in recs]))
    z = coeff_words([5, 6, 7])
    verdict = np.zeros(3, np.uint8)
    box, t, other = w.box(), v.Tally(ctx, w.el.n + 2), v.Tally(ctx, w.el.n + 3)
    try:
        seen = receive(box, w.pool[10:12], None, t)
        assert seen["verdict"] == [1, 1]
        before, serials = t.result(), box.serials()
        ctx.stats_reset()
        call = lib.vsp_ballot_box_receive_blobs
        for args in ((None, t.h, p(ct), p(pr), p(inp), 3), (box.h, t.h, None, p(pr), p(inp), 3), (box.h, t.h, p(ct), None, p(inp), 3), (box.h, t.h, p(ct), p(pr), None, 3),
                     (box.h, other.h, p(ct), p(pr), p(inp), 3), (box.h, t.h, None, None, None, 0)):
            for coeff in (p(z), None):
                assert call(ctx.h, *args, 1, coeff, p(verdict), None, None, None, None) == ERR_ARG, args
        assert call(ctx.h, box.h, t.h, p(ct), p(pr), p(inp), 3, 1, p(z), None, None, None, None, None) == ERR_ARG
        assert call(ctx.h, box.h, t.h, p(ct), p(pr), p(inp), 3, 1, p(coeff_words([5, 0, 7])), p(verdict), None, None, None, None) == ERR_ARG
        assert "zero" in ctx.last_error()
        bad = serial_rows([(1, 2), (3, R)])
        assert lib.vsp_ballot_box_add_serials(ctx.h, box.h, p(bad), 2, None, None) == ERR_ARG and "below r" in ctx.last_error()
        assert lib.vsp_ballot_box_add_serials(ctx.h, None, p(bad), 2, None, None) == ERR_ARG
        out = np.zeros((3, 2, 4), np.uint64)
        assert lib.vsp_ballot_box_serials(ctx.h, box.h, 1, 2, p(out)) == ERR_ARG and lib.vsp_ballot_box_serials(ctx.h, box.h, 0, 2, None) == ERR_ARG
        # all of it before any GPU work, and nothing touched
        assert int(ctx.stat("saver_receive_ballots")) == 0 and ctx.stat("ballot_box_ms") == 0
        after = t.result()
        assert np.array_equal(before[0], after[0]) and before[1] == after[1] == 2
        assert box.count() == 2 and np.array_equal(box.serials(), serials)
        accepted = C.c_size_t(7)
        assert call(ctx.h, box.h, t.h, p(ct), p(pr), p(inp), 0, 1, p(z), p(verdict), None, None, C.byref(accepted), None) == 0 and accepted.value == 0
        with pytest.raises(ValueError):
            box.receive_blobs([r.ct for r in recs], [r.pr for r in recs[:2]], [r.inp for r in recs])
        # a following good call gives the model's result
        batch = list(recs) + [w.pool[10]]
        for mode in MODES:
            got = receive(box, batch, coeffs_for(mode, 1010, 4), t)
            first = mode == "exact"
            assert got["verdict"] == [int(first)] * 3 + [0] and got["reason"] == [0 if first else 16] * 3 + [16]
            assert got["holder"] == ([NONE] * 3 if first else [2, 3, 4]) + [0]
        want = tally_of(ctx, w.el.n + 2, [r.ct for r in w.pool[10:12]] + [r.ct for r in recs])
        got = t.result()
        assert np.array_equal(got[0], want[0]) and got[1] == want[1] == 5 and box.count() == 5
    finally:
        box.free(); t.free(); other.free()
