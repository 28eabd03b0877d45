"""CPU build of the device square root in Fp2: vote_saver_protocol_amd/csrc/fp2_sqrt.h compiled by g++ with the 32-bit-limb type the
G2 decoding kernel uses (and the host's 64-bit-limb type), checked against the oracle's fp2_sqrt and the oracle's point compression.
No GPU, no HIP."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bls12_381 as o
from conftest import I, L, ROOT

P = o.P
F2 = o.Fp2Ops
H = (P - 1) // 2
B2 = (4, 4)


@pytest.fixture(scope="module")
def sc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cpu_build") / "libsqrt2chk.so")
    flags = os.environ.get("VSP_MATHCHK_FLAGS", "-O2").split()
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-shared", "-fPIC", "-o", so,
                           os.path.join(ROOT, "tests", "cpu_build", "sqrt2_check.cpp")])
    return C.CDLL(so)


def limbs2(a):
    return np.concatenate([L(a[0], 6), L(a[1], 6)])


def root(lib, fn, a):
    out = np.zeros(12, np.uint64)
    ok = getattr(lib, fn)(limbs2(a).ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return (I(out[:6]), I(out[6:])), bool(ok)


def y_of(lib, fn, x, larger):
    out = np.zeros(12, np.uint64)
    ok = getattr(lib, fn)(limbs2(x).ctypes.data_as(C.c_void_p), int(larger), out.ctypes.data_as(C.c_void_p))
    return (I(out[:6]), I(out[6:])), bool(ok)


def rand_fp(gen):
    a = 0
    for _ in range(6):
        a = (a << 64) | next(gen)
    return a % P


def is_square(a):
    """a square in Fp2 exactly when the norm is a square in Fp"""
    n = (a[0] * a[0] + a[1] * a[1]) % P
    return n == 0 or pow(n, H, P) == 1


def samples():
    """(squares, non-squares): the fixed values, the generator's right-hand side, values with c1 = 0 (c0 a residue and not) and with
    c0 = 0, and 64 random squares and 64 random non-squares"""
    gx, _ = o.G2.gen
    fixed = [(0, 0), (1, 0), (0, 1), (P - 1, 0), B2, F2.add(F2.mul(F2.sqr(gx), gx), B2)]
    gen = o.splitmix64(2025)
    res_c0 = next(a for a in iter(lambda: rand_fp(gen), None) if pow(a, H, P) == 1)
    non_c0 = next(a for a in iter(lambda: rand_fp(gen), None) if pow(a, H, P) == P - 1)
    fixed += [(res_c0, 0), (non_c0, 0), (4, 0), (P - 4, 0), (0, res_c0), (0, non_c0), (0, P - 1), (0, 2)]
    sq, non = [], []
    while len(sq) < 64 or len(non) < 64:
        a = (rand_fp(gen), rand_fp(gen))
        if is_square(a) and len(sq) < 64:
            sq.append(a)
        elif not is_square(a) and len(non) < 64:
            non.append(a)
    for a in fixed:
        (sq if is_square(a) else non).append(a)
    return sq, non


@pytest.mark.parametrize("fn", ["chk_fp2_sqrt", "chk_hfp2_sqrt"])
def test_square_root_and_verdict(sc, fn):
    sq, non = samples()
    assert len(non) > 64                                            # 4 (1 + u) is no square: x = 0 has no point
    for a in sq:
        want = o.fp2_sqrt(a)
        got, ok = root(sc, fn, a)
        assert want is not None and ok, a
        assert got[0] < P and got[1] < P
        assert F2.sqr(got) == a and got in (want, F2.neg(want)), a   # either root
    for a in non:
        assert o.fp2_sqrt(a) is None
        assert not root(sc, fn, a)[1], a
    assert root(sc, fn, (0, 0)) == ((0, 0), True)
    # every element of Fp is a square in Fp2: c1 = 0 with c0 not a residue has a root on the u axis
    a = next(a for a in sq if a[1] == 0 and a[0] and pow(a[0], H, P) == P - 1)
    assert root(sc, fn, a)[0][0] == 0


@pytest.mark.parametrize("fn", ["chk_fp2_larger", "chk_hfp2_larger"])
def test_sign_rule_boundaries(sc, fn):
    cases = [((0, 0), False), ((H, 0), False), ((H + 1, 0), True), ((1, 0), False), ((P - 1, 0), True),
             ((0, H), False), ((0, H + 1), True), ((P - 1, H), False), ((P - 1, 1), False), ((1, P - 1), True),
             ((H + 1, 1), False), ((H, P - 1), True)]
    for a, want in cases:
        assert bool(getattr(sc, fn)(limbs2(a).ctypes.data_as(C.c_void_p))) == want, a
        assert o._lex_larger_fp2(a) == want, a


@pytest.mark.parametrize("fn", ["chk_g2_y", "chk_hg2_y"])
def test_sign_selection_matches_the_oracle_codec(sc, fn):
    """the y the decoder picks for P and for -P is the one the oracle's g2_decompress picks from the oracle's g2_compress bytes"""
    gen = o.splitmix64(7)
    for k in [1, 2, 3, o.R - 1] + [o.rand_fr(gen) for _ in range(12)]:
        Pt = o.G2.mul(o.G2.gen, k)
        for Q in (Pt, o.G2.neg(Pt)):
            enc = o.g2_compress(Q)
            larger = bool(enc[0] & 0x20)
            assert o.g2_decompress(enc) == Q
            y, ok = y_of(sc, fn, Q[0], larger)
            assert ok and y == Q[1]
            y2, ok2 = y_of(sc, fn, Q[0], not larger)
            assert ok2 and y2 == F2.neg(Q[1])
    # abscissas with no point: the verdict is false for either flag
    for x in ((0, 0), (1, 0)):
        assert o.fp2_sqrt(F2.add(F2.mul(F2.sqr(x), x), B2)) is None
        assert not y_of(sc, fn, x, False)[1] and not y_of(sc, fn, x, True)[1]


# ---- the decoding rules around the root: point_decode.h decode_record on 96-byte records, as the decoding kernel runs it
@pytest.fixture(scope="module")
def dc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cpu_build") / "libdecodechk.so")
    flags = os.environ.get("VSP_MATHCHK_FLAGS", "-O2").split()
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-shared", "-fPIC", "-o", so,
                           os.path.join(ROOT, "tests", "cpu_build", "decode_check.cpp")])
    return C.CDLL(so)


ZERO2 = ((0, 0), (0, 0))


def decode2(lib, rec):
    out = np.zeros(24, np.uint64)
    st = lib.chk_decode_g2(bytes(rec), out.ctypes.data_as(C.c_void_p))
    return st, ((I(out[:6]), I(out[6:12])), (I(out[12:18]), I(out[18:])))


def want2(rec):
    """status and point by the oracle codec.  What it refuses (an assertion) is status 2 when the record is well formed -- compressed,
    finite, both coefficients < p -- and only the curve has no such point, status 1 otherwise"""
    try:
        pt = o.g2_decompress(bytes(rec))
    except AssertionError:
        x = (int.from_bytes(rec[48:96], "big"), int.from_bytes(bytes([rec[0] & 0x1F]) + bytes(rec[1:48]), "big"))
        well_formed = (rec[0] & 0xC0) == 0x80 and x[0] < P and x[1] < P
        assert not well_formed or not is_square(F2.add(F2.mul(F2.sqr(x), x), B2))
        return (2 if well_formed else 1), ZERO2
    return 0, (pt if pt is not None else ZERO2)


def rec2(x, flags=0x80):
    b = bytearray(x[1].to_bytes(48, "big") + x[0].to_bytes(48, "big"))
    b[0] |= flags
    return bytes(b)


def test_decode_record_accepts_what_the_oracle_codec_writes(dc):
    gen = o.splitmix64(11)
    signs = set()
    for k in [1, 2, o.R - 1] + [o.rand_fr(gen) for _ in range(12)]:
        Pt = o.G2.mul(o.G2.gen, k)
        for Q in (Pt, o.G2.neg(Pt)):
            enc = o.g2_compress(Q)
            signs.add(enc[0] & 0x20)
            assert decode2(dc, enc) == (0, Q) == want2(enc)
    assert signs == {0, 0x20}
    inf = o.g2_compress(None)
    assert inf == bytes([0xC0]) + bytes(95) and decode2(dc, inf) == (0, ZERO2) == want2(inf)


def test_decode_record_rejections(dc):
    gx = o.G2.mul(o.G2.gen, 5)[0]
    good = o.g2_compress(o.G2.mul(o.G2.gen, 5))
    malformed = [bytes([0xE0]) + bytes(95), bytes([0xC0]) + bytes(94) + b"\x01", bytes([0xC0]) + bytes(46) + b"\x01" + bytes(48),
                 bytes([good[0] & 0x7F]) + good[1:], rec2((P, P)), rec2((gx[0], P)), rec2((P, gx[1])), rec2((gx[0], P), 0xA0)]
    for rec in malformed:
        assert decode2(dc, rec) == (1, ZERO2) == want2(rec), rec.hex()
    # p - 1 is canonical in either coefficient: the verdict is the curve's
    for x in ((P - 1, 0), (0, P - 1), (P - 1, P - 1)):
        has_point = o.fp2_sqrt(F2.add(F2.mul(F2.sqr(x), x), B2)) is not None
        for flags in (0x80, 0xA0):
            st, pt = decode2(dc, rec2(x, flags))
            assert (st, pt) == want2(rec2(x, flags)) and st == (0 if has_point else 2)
    # abscissas with no point
    for x in ((0, 0), (1, 0)):
        for flags in (0x80, 0xA0):
            assert decode2(dc, rec2(x, flags)) == (2, ZERO2) == want2(rec2(x, flags))
