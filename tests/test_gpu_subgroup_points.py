"""GPU: k_subgroup_check (csrc/msm_impl.inc) on curve points of every small cofactor order, through every caller that relies on it.
The points are tests/golden/cofactor_points.json (oracle/gen_golden.py cofactor_points(): T_q of each small prime order q of the two
cofactors, -T_q, S + T_q for a subgroup point S, and S); the expected verdict of each is the oracle's multiplication by r, which
tests/test_subgroup_model_cpu.py checks against the fixture and against a model of the kernel's ladder.  Every G1 T_q has
lambda T_q = O: the kernel's running multiple ends at infinity and its `inf2` term alone rejects the point; a point of order 3 or 11
walks the ladder through its exceptional additions on the way.  All verdicts here are exact."""
import numpy as np
import pytest

import bls12_381 as o
import wire
from conftest import dec1, dec2, g1_limbs, g2_limbs, load_golden, rand_fr_array

import dlog_election as de
from test_gpu_saver_receive import Case, receive, tally_of as receive_tally_of, with_member
from test_gpu_tally import oracle_sum, tally_of

import vote_saver_protocol_amd as v

pytestmark = pytest.mark.gpu


class Points:
    """the fixture, decoded: per group the records' labels, points, compressed bytes and verdicts, and a pool of subgroup points"""

    def __init__(self, cref):
        fx = load_golden("cofactor_points.json")
        self.g = {}
        for group, name, dec, comp, limbs, batch, width in ((1, "g1", dec1, o.g1_compress, g1_limbs, cref.g1_batch_mul_gen, 12),
                                                            (2, "g2", dec2, o.g2_compress, g2_limbs, cref.g2_batch_mul_gen, 24)):
            recs = fx[name]
            pts = [dec(r["point"]) for r in recs]
            good = batch(rand_fr_array(130, 20280 + group))
            self.g[group] = dict(label=[r["label"] for r in recs], pt=pts, enc=[comp(p) for p in pts], inside=[r["in_subgroup"] for r in recs],
                                 limbs=np.array([limbs(p) for p in pts], np.uint64), good=good, width=width,
                                 good_enc=[(v.g1_compress if group == 1 else v.g2_compress)(row) for row in good])

    def by_label(self, group, label):
        g = self.g[group]
        return g["pt"][g["label"].index(label)]

    def bad(self, group):
        g = self.g[group]
        return [i for i in range(len(g["pt"])) if not g["inside"][i]]


@pytest.fixture(scope="module")
def points(cref):
    p = Points(cref)
    assert len(p.bad(1)) == 15 and len(p.bad(2)) == 18 and p.by_label(1, "T_3") == (0, 2)
    return p


def host_verdict(fn, enc, check_subgroup):
    try:
        fn(enc, check_subgroup=check_subgroup)
        return True
    except ValueError:
        return False


# ---------------------------------------------------------------------------------------------- 1. decompression batches
# G1: one lane per point, 64 points a wave: lanes 0, 63 and the next wave's 0 (point 64), pairs of bad neighbours (1-2, 62-63-64-65), bad
# points with good ones on both sides, the last wave's first two lanes (128, 129).  G2: a lane pair per point, 32 points a wave: the first
# pair (0), the last (31), the next wave's first (32), and the third wave's two points (64, 65)
PLACES = {1: (130, (0, 1, 2, 17, 40, 62, 63, 64, 65, 67, 100, 126, 127, 128, 129, 5)),
          2: (66, (0, 1, 3, 10, 16, 30, 31, 32, 33, 35, 40, 47, 48, 50, 62, 63, 64, 65, 20))}


@pytest.mark.parametrize("rot", [0, 5, 10])
@pytest.mark.parametrize("group", [1, 2])
def test_decompression_batches_reject_exactly_the_points_outside_the_subgroup(ctx, points, group, rot):
    """every fixture point of the group (S too) among subgroup points; `rot` moves other fixture points onto the waves' edges"""
    g = points.g[group]
    n, places = PLACES[group]
    k = len(g["pt"])
    assert len(places) == k and len(set(places)) == k and max(places) < n
    encs, want, inside = list(g["good_enc"][:n]), [0] * n, {}
    for j, at in enumerate(places):
        i = (j + rot) % k
        encs[at], want[at], inside[at] = g["enc"][i], 0 if g["inside"][i] else 4, i
    assert {want[a] for a in ((0, 63, 64) if group == 1 else (0, 31, 32))} == {4}
    batch, host = (v.g1_decompress_batch, v.g1_decompress) if group == 1 else (v.g2_decompress_batch, v.g2_decompress)
    for at in places:                                                          # the host function's verdict on the same bytes
        assert host_verdict(host, encs[at], True) == (want[at] == 0), g["label"][inside[at]]
    out, status = batch(ctx, b"".join(encs), check_subgroup=True)
    assert status.tolist() == want
    for at in range(n):
        if want[at]:
            assert not out[at].any()
        else:
            assert np.array_equal(out[at], g["limbs"][inside[at]] if at in inside else g["good"][at])
    out, status = batch(ctx, b"".join(encs), check_subgroup=False)
    assert not status.any()
    for at in range(n):
        if at in inside:
            assert np.array_equal(out[at], host(encs[at], check_subgroup=False)) and np.array_equal(out[at], g["limbs"][inside[at]])
        else:
            assert np.array_equal(out[at], g["good"][at])


# ---------------------------------------------------------------------------------------------- 2. the flag form: strict uploads
def test_strict_uploads_refuse_every_fixture_point_at_the_waves_edges(points):
    with v.Context(0) as cx:
        cx.set_option("bases_check_subgroup", 2)
        checks = refused = 0
        for group, edges in ((1, (0, 63, 64)), (2, (0, 31, 32, 63, 64))):
            g = points.g[group]
            good = g["good"][:65]
            bad = points.bad(group)
            for j, i in enumerate(bad):                                        # each point outside the subgroup at one of the edges, by turns
                bases = good.copy()
                bases[edges[j % len(edges)]] = g["limbs"][i]
                with pytest.raises(v.VspError, match="subgroup"):
                    cx.upload_bases(bases, group)
                checks += 1; refused += 1
            for at in edges:                                                   # and one point at every edge: T_3 / T_13
                bases = good.copy()
                bases[at] = g["limbs"][0]
                with pytest.raises(v.VspError, match="subgroup"):
                    cx.upload_bases(bases, group)
                checks += 1; refused += 1
            for i in bad:                                                      # alone
                if g["label"][i].startswith("T_"):
                    with pytest.raises(v.VspError, match="subgroup"):
                        cx.upload_bases(g["limbs"][i:i + 1], group)
                    checks += 1; refused += 1
            B = cx.upload_bases(good, group)                                   # the same 65 good points
            checks += 1
            B.free()
            assert cx.stat("bases_subgroup_checks") == checks and cx.stat("bases_outside_subgroup") == refused
        assert refused == 15 + 3 + 5 + 18 + 5 + 6


# ---------------------------------------------------------------------------------------------- 3. callers with their own status plumbing
def test_proof_blobs_with_a_small_order_member_are_rejected(ctx, points):
    g1, g2 = points.g[1], points.g[2]
    good = [g1["good_enc"][k] + g2["good_enc"][k] + g1["good_enc"][65 + k] for k in range(5)]
    member = {"A": (0, 48, 0x10), "B": (48, 144, 0x20), "C": (144, 192, 0x40)}
    for name, enc in (("A", o.g1_compress(points.by_label(1, "T_3"))), ("B", o.g2_compress(points.by_label(2, "T_13"))),
                      ("C", o.g1_compress(points.by_label(1, "S+T_11")))):
        lo, hi, bit = member[name]
        blobs = list(good)
        blobs[2] = blobs[2][:lo] + enc + blobs[2][hi:]
        assert not host_verdict(v.proof_from_blob, blobs[2], True) and host_verdict(v.proof_from_blob, blobs[2], False)
        A, B, Cc, status = v.proofs_from_blob_batch(ctx, b"".join(blobs), check_subgroup=True)
        assert status.tolist() == [0, 0, 4 | bit, 0, 0], name
        assert not A[2].any() and not B[2].any() and not Cc[2].any()
        for k in (0, 1, 3, 4):
            assert np.array_equal(A[k], g1["good"][k]) and np.array_equal(B[k], g2["good"][k]) and np.array_equal(Cc[k], g1["good"][65 + k])


def test_tally_rejects_a_ballot_whose_element_carries_an_order_3_component(ctx, points):
    T3 = points.by_label(1, "T_3")
    cts = [[o.g1_from_limbs([int(t) for t in points.g[1]["good"][3 * b + j]]) for j in range(3)] for b in range(6)]
    sent = [list(ct) for ct in cts]
    sent[4][1] = o.G1.add(cts[4][1], T3)
    assert o.G1.is_on_curve(sent[4][1]) and not o.G1.in_subgroup(sent[4][1])
    status, accepted, ct, ballots = tally_of(ctx, 3, [wire.g1_vector(c) for c in sent])
    assert status.tolist() == [0, 0, 0, 0, 4, 0] and accepted == ballots == 5
    assert np.array_equal(ct, oracle_sum([cts[b] for b in (0, 1, 2, 3, 5)]))
    sent[1][2] = points.by_label(1, "-T_11")                                   # and a pure small-order element: lambda P = O
    status, accepted, ct, ballots = tally_of(ctx, 3, [wire.g1_vector(c) for c in sent])
    assert status.tolist() == [0, 4, 0, 0, 4, 0] and accepted == ballots == 4
    assert np.array_equal(ct, oracle_sum([cts[b] for b in (0, 2, 3, 5)]))


# ---------------------------------------------------------------------------------------------- 4. the attack include/vsp.h describes
def test_receive_rejects_an_order_3_component_under_a_coefficient_divisible_by_3(ctx, cref, points):
    """a valid ballot whose ct_1 carries T_3, screened under a coefficient that is a multiple of 3 (3 z T_3 = O: the combination alone would
    not see it): with the subgroup check the decoder rejects it on the wire, whatever the coefficient"""
    c = Case(ctx, 800, 2, 1, 6)
    try:
        b = c.valid.cut(slice(0, 6))
        at = 3
        limbs = v.g1_decompress(b.ct[at][8 + 48:8 + 96])
        ct1 = o.g1_from_limbs([int(t) for t in limbs])
        moved = o.G1.add(ct1, points.by_label(1, "T_3"))
        assert o.G1.is_on_curve(moved) and not o.G1.in_subgroup(moved) and o.G1.mul(moved, 3) == o.G1.mul(ct1, 3)
        b.ct[at] = with_member(b.ct[at], 1, o.g1_compress(moved))
        rng = de.rng(880)
        zs = [rng.randrange(1, 1 << 128) for _ in range(6)]
        zs[at] = 3 * rng.randrange(1, 1 << 126)
        got = receive(ctx, c, b, zs, check=True)
        assert got["wire"] == [[4 if k == at else 0, 0, 0] for k in range(6)]
        assert got["verdict"] == [int(k != at) for k in range(6)] and got["reason"] == [int(k == at) for k in range(6)]
        assert got["accepted"] == 5
        others = receive_tally_of(ctx, c.el.n + 2, [b.ct[k] for k in range(6) if k != at])
        assert np.array_equal(got["tally"][0], others[0]) and got["tally"][1] == others[1] == 5
    finally:
        c.ver.free()
