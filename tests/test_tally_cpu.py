"""CPU build of the device square root: vote_saver_protocol_amd/csrc/fp_sqrt.h compiled by g++ with the 32-bit-limb type the
decoding kernel of the tally uses (and the host's 64-bit-limb type), checked against pow(a, (p+1)/4, p) and the oracle's point
compression.  No GPU, no HIP."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bls12_381 as o
from conftest import I, L, ROOT

P = o.P
E = (P + 1) // 4


@pytest.fixture(scope="module")
def sc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cpu_build") / "libsqrtchk.so")
    flags = os.environ.get("VSP_MATHCHK_FLAGS", "-O2").split()
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-shared", "-fPIC", "-o", so,
                           os.path.join(ROOT, "tests", "cpu_build", "sqrt_check.cpp")])
    return C.CDLL(so)


def root(lib, fn, a):
    out = np.zeros(6, np.uint64)
    ok = getattr(lib, fn)(L(a, 6).ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return I(out), bool(ok)


def y_of(lib, fn, x, larger):
    out = np.zeros(6, np.uint64)
    ok = getattr(lib, fn)(L(x, 6).ctypes.data_as(C.c_void_p), int(larger), out.ctypes.data_as(C.c_void_p))
    return I(out), bool(ok)


def samples():
    """fixed values, the generator's right-hand side, 64 random residues and 64 random non-residues"""
    gx, _ = o.G1.gen
    vals = [0, 1, 4, P - 1, (gx * gx * gx + 4) % P]
    gen = o.splitmix64(2024)
    res, non = [], []
    while len(res) < 64 or len(non) < 64:
        a = 0
        for _ in range(6):
            a = (a << 64) | next(gen)
        a %= P
        if a == 0:
            continue
        is_res = pow(a, (P - 1) // 2, P) == 1
        if is_res and len(res) < 64:
            res.append(a)
        elif not is_res and len(non) < 64:
            non.append(a)
    return vals, res, non


@pytest.mark.parametrize("fn", ["chk_fp_sqrt", "chk_hfp_sqrt"])
def test_square_root_and_verdict(sc, fn):
    vals, res, non = samples()
    for a in vals + res + non:
        want = pow(a, E, P)
        got, ok = root(sc, fn, a)
        assert got == want, hex(a)
        assert ok == (want * want % P == a), hex(a)
    assert all(root(sc, fn, a)[1] for a in res + [0, 1, 4])
    assert not any(root(sc, fn, a)[1] for a in non + [P - 1])        # p = 3 mod 4: -1 is not a square


def test_above_half_boundary(sc):
    h = (P - 1) // 2
    for a, want in ((0, False), (1, False), (h - 1, False), (h, False), (h + 1, True), (P - 1, True), (1 << 380, True), ((1 << 352) - 1, False)):
        assert bool(sc.chk_fp_above_half(L(a, 6).ctypes.data_as(C.c_void_p))) == want, hex(a)


@pytest.mark.parametrize("fn", ["chk_g1_y", "chk_hg1_y"])
def test_sign_selection_matches_the_oracle_codec(sc, fn):
    """the y the decoder picks for P and for -P is the one the oracle's g1_decompress picks from the oracle's g1_compress bytes"""
    gen = o.splitmix64(7)
    for k in [1, 2, 3, o.R - 1] + [o.rand_fr(gen) for _ in range(12)]:
        Pt = o.G1.mul(o.G1.gen, k)
        for Q in (Pt, o.G1.neg(Pt)):
            enc = o.g1_compress(Q)
            larger = bool(enc[0] & 0x20)
            assert o.g1_decompress(enc) == Q
            y, ok = y_of(sc, fn, Q[0], larger)
            assert ok and y == Q[1]
            y2, ok2 = y_of(sc, fn, Q[0], not larger)
            assert ok2 and y2 == P - Q[1]
    # an abscissa with no point: the verdict is false for either flag
    x = next(x for x in range(2, 100) if pow((x ** 3 + 4) % P, (P - 1) // 2, P) != 1)
    assert not y_of(sc, fn, x, False)[1] and not y_of(sc, fn, x, True)[1]


# ---- the decoding rules around the root: point_decode.h decode_record, as the decoding kernel runs it
DECODE_SRC = os.path.join(ROOT, "tests", "cpu_build", "decode_check.cpp")


@pytest.fixture(scope="module")
def dc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cpu_build") / "libdecodechk.so")
    flags = os.environ.get("VSP_MATHCHK_FLAGS", "-O2").split()
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-shared", "-fPIC", "-o", so, DECODE_SRC])
    return C.CDLL(so)


def decode1(lib, rec):
    out = np.zeros(12, np.uint64)
    st = lib.chk_decode_g1(bytes(rec), out.ctypes.data_as(C.c_void_p))
    return st, (I(out[:6]), I(out[6:]))


def want1(rec):
    """status and point by the oracle codec.  What it refuses (an assertion) is status 2 when the record is well formed -- compressed,
    finite, x < p -- and only the curve has no such point, status 1 otherwise"""
    try:
        pt = o.g1_decompress(bytes(rec))
    except AssertionError:
        x = int.from_bytes(bytes([rec[0] & 0x1F]) + bytes(rec[1:]), "big")
        well_formed = (rec[0] & 0xC0) == 0x80 and x < P
        assert not well_formed or pow((x ** 3 + 4) % P, (P - 1) // 2, P) == P - 1
        return (2 if well_formed else 1), (0, 0)
    return 0, (pt if pt is not None else (0, 0))


def rec1(x, flags=0x80):
    b = bytearray(x.to_bytes(48, "big"))
    b[0] |= flags
    return bytes(b)


def test_decode_record_accepts_what_the_oracle_codec_writes(dc):
    gen = o.splitmix64(11)
    signs = set()
    for k in [1, 2, o.R - 1] + [o.rand_fr(gen) for _ in range(12)]:
        Pt = o.G1.mul(o.G1.gen, k)
        for Q in (Pt, o.G1.neg(Pt)):
            enc = o.g1_compress(Q)
            signs.add(enc[0] & 0x20)
            assert decode1(dc, enc) == (0, Q) == want1(enc)
    assert signs == {0, 0x20}
    inf = o.g1_compress(None)
    assert inf == bytes([0xC0]) + bytes(47) and decode1(dc, inf) == (0, (0, 0)) == want1(inf)


def test_decode_record_rejections(dc):
    good = o.g1_compress(o.G1.mul(o.G1.gen, 5))
    malformed = [bytes([0xE0]) + bytes(47), bytes([0xC0]) + bytes(46) + b"\x01", bytes([good[0] & 0x7F]) + good[1:], rec1(P), rec1(P, 0xA0)]
    for rec in malformed:
        assert decode1(dc, rec) == (1, (0, 0)) == want1(rec), rec.hex()
    # x = p - 1 is canonical: the verdict is the curve's
    for flags in (0x80, 0xA0):
        rec = rec1(P - 1, flags)
        has_point = pow(((P - 1) ** 3 + 4) % P, (P - 1) // 2, P) == 1
        st, pt = decode1(dc, rec)
        assert (st, pt) == want1(rec) and st == (0 if has_point else 2)
    # the first small x with no point
    x = next(x for x in range(2, 100) if pow((x ** 3 + 4) % P, (P - 1) // 2, P) != 1)
    for flags in (0x80, 0xA0):
        assert decode1(dc, rec1(x, flags)) == (2, (0, 0)) == want1(rec1(x, flags))


def test_decode_check_stand_alone_under_sanitizers(tmp_path):
    """decode_check.cpp with its own main under AddressSanitizer and UBSan: both groups, no code loaded into python"""
    exe = str(tmp_path / "decode_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DDECODE_CHECK_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, DECODE_SRC])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "decode_check: ok" in p.stdout, p.stdout + p.stderr
