"""CPU build of the rules of receiving ballots from their blobs: vote_saver_protocol_amd/csrc/receive.h compiled by g++.  The input
blob's acceptance rule -- the one k_receive_scalars applies lane by lane -- against vsp_fr_vector_from_blob (host code of the library)
on r - 1, r, 2^256 - 1, wrong headers and short counts, and the decoded words against the host decoder's; the index maps between the
decoder's ballot-major layout and the verifiers' columns for pieces of 1, 63, 64 and 65 ballots and for ranges inside a piece.  No
GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bls12_381 as o
from conftest import ROOT, I

import vote_saver_protocol_amd as v

SRC = os.path.join(ROOT, "tests", "cpu_build", "receive_check.cpp")
R = o.R


@pytest.fixture(scope="module")
def rc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cpu_build") / "librecvchk.so")
    flags = os.environ.get("VSP_MATHCHK_FLAGS", "-O2").split()
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    lib = C.CDLL(so)
    for name in ("chk_input_blob_bytes", "chk_wire_stride", "chk_scalar_lanes"):
        getattr(lib, name).restype = C.c_size_t
    return lib


def blob_of(count, values):
    return count.to_bytes(8, "big") + b"".join(x.to_bytes(32, "big") for x in values)


def rule(lib, blob, n_rest):
    """-> (status byte, the decoded scalars as integers) of the header rule"""
    buf = np.array(list(blob), dtype=np.uint8)
    out = np.zeros((max(n_rest, 1), 8), np.uint32)
    st = lib.chk_input_blob(buf.ctypes.data_as(C.c_void_p), C.c_size_t(n_rest), out.ctypes.data_as(C.c_void_p))
    return st, [sum(int(w) << (32 * i) for i, w in enumerate(row)) for row in out[:n_rest]]


def host_accepts(blob, n_rest):
    """vsp_fr_vector_from_blob accepts the blob with a count of exactly n_rest"""
    try:
        vals = v.fr_vector_from_blob(blob)
    except ValueError:
        return False, None
    return vals.shape[0] == n_rest, [I(x) for x in vals]


EDGE = [0, 1, R - 1, R, R + 1, (1 << 255) - 1, 1 << 255, (1 << 256) - 1, 0x0123456789abcdef_fedcba9876543210_0f1e2d3c4b5a6978_8796a5b4c3d2e1f0 % R]


@pytest.mark.parametrize("n_rest", [1, 2, 5])
def test_the_scalar_rule_is_the_host_decoders(rc, n_rest):
    assert rc.chk_input_blob_bytes(n_rest) == len(blob_of(n_rest, [0] * n_rest)) == len(v.fr_vector_to_blob(np.zeros((n_rest, 4), np.uint64)))
    for at in range(n_rest):
        for x in EDGE:
            vals = [(7 + i) % R for i in range(n_rest)]
            vals[at] = x
            blob = blob_of(n_rest, vals)
            ok, host_vals = host_accepts(blob, n_rest)
            st, got = rule(rc, blob, n_rest)
            assert ok == (x < R) and st == (0 if ok else 1), (at, hex(x))
            assert got == vals                                       # the words are the scalar's, accepted or not
            if ok:
                assert got == host_vals


def test_wrong_headers_and_short_counts(rc):
    vals = [R - 1, 5, 6]
    good = blob_of(3, vals)
    assert rule(rc, good, 3)[0] == 0 and host_accepts(good, 3)[0]
    assert v.fr_vector_to_blob(np.array([[(x >> (64 * i)) & (2**64 - 1) for i in range(4)] for x in vals], np.uint64)) == good
    # the header names another count than the verifier's key: the blob has the length the receive call gives every ballot, 8 + 32 n_rest
    for count in (0, 2, 4, 1 << 32, 3 << 56, (1 << 64) - 1, 3 | (1 << 63)):
        blob = blob_of(count, vals)
        assert rule(rc, blob, 3)[0] == 1, count
        assert not host_accepts(blob, 3)[0], count
    # a blob that is a well-formed vector of fewer scalars is a short count for this key
    short = blob_of(2, vals[:2])
    assert host_accepts(short, 2)[0] and not host_accepts(short, 3)[0]
    assert rule(rc, short + bytes(32), 3)[0] == 1
    # no rest inputs: the header alone, which must say zero
    assert rule(rc, blob_of(0, []), 0)[0] == 0 and host_accepts(blob_of(0, []), 0)[0]
    assert rule(rc, blob_of(1, []), 0)[0] == 1 and not host_accepts(blob_of(1, []), 0)[0]
    assert rc.chk_scalar_lanes(0) == 1 and rc.chk_scalar_lanes(1) == 1 and rc.chk_scalar_lanes(5) == 5


def gather(lib, pc, n, lo, c):
    out = np.full((n + 5) * c, -7, np.int64)
    bad = lib.chk_gather(C.c_size_t(pc), C.c_size_t(n), C.c_size_t(lo), C.c_size_t(c), out.ctypes.data_as(C.c_void_p))
    return bad, out


@pytest.mark.parametrize("n", [1, 2, 25])
@pytest.mark.parametrize("pc,lo,c", [(1, 0, 1), (63, 0, 63), (64, 0, 64), (65, 0, 65), (65, 64, 1), (130, 33, 64), (130, 65, 65), (130, 98, 32), (130, 129, 1)])
def test_index_maps_between_the_ballot_major_and_the_column_layout(rc, n, pc, lo, c):
    """every entry of the verifier's piece is written once, from inside the decoded piece, and is the point k_ballot_prepare puts
    there: argument j of ballot k at j c + k, acc at column n + 2, C at n + 3, then A"""
    bad, out = gather(rc, pc, n, lo, c)
    assert bad == 0
    members = np.arange(pc * (n + 2)).reshape(pc, n + 2)             # point numbers, ballot-major
    base = pc * (n + 2)
    want = np.concatenate([members[lo:lo + c].T.reshape(-1), np.full(c, -1), base + pc + np.arange(lo, lo + c), base + np.arange(lo, lo + c)])
    assert np.array_equal(out, want)


def test_wire_status_stride_keeps_the_three_arrays_word_aligned(rc):
    for pc in (1, 2, 3, 4, 5, 63, 64, 65, 130, 1 << 16):
        s = rc.chk_wire_stride(pc)
        assert s >= pc and s % 4 == 0 and s - pc < 4


def test_stand_alone_program_under_sanitizers(tmp_path):
    """receive_check.cpp with its own main under AddressSanitizer and UBSan: no code loaded into python"""
    exe = str(tmp_path / "receive_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DRECEIVE_CHECK_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "receive_check: ok" in p.stdout, p.stdout + p.stderr
