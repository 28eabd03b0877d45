"""CPU build of the voting circuit's rules: vote_saver_protocol_amd/csrc/vote_circuit.h compiled by g++ (64-bit limbs) at depth 2,
eid_bits 5, n 3, g 3.  The header's host path builds witnesses; every row of the matrices the header's builder made is evaluated on them
in 64-bit limbs and, over the exported CSR, by the big-integer judge of tests/vote_circuit_model.py, which also supplies the protocol's
public inputs.  No GPU."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import jubjub_model as jm
import vote_circuit_model as vm
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpu_build", "vote_circuit_check.cpp")
G, N, EID_BITS, DEPTH = 3, 3, 5, 2
M, EID_PACKED, SN_PACKED, RT_PACKED, EID, SK, ADDRESS, COPATH, SN_BITS, RT_BITS = range(10)


def p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cpu_build") / "libvcchk.so")
    flags = os.environ.get("VSP_MATHCHK_FLAGS", "-O2").split()
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.chk_vc_new.restype = C.c_void_p
    lib.chk_vc_new.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int]
    lib.chk_vc_free.argtypes = [C.c_void_p]
    lib.chk_vc_sizes.argtypes = [C.c_void_p, C.c_void_p]
    lib.chk_vc_csr.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.chk_vc_wires.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.chk_vc_columns_ok.argtypes = [C.c_void_p]
    lib.chk_vc_witness.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.chk_vc_first_bad_row.restype = C.c_uint64
    lib.chk_vc_first_bad_row.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def gens():
    return jm.generators(G)


@pytest.fixture(scope="module")
def table(gens):
    return jm.Table(gens)


class Circuit:
    def __init__(self, lib, gens, hash_leaves):
        self.lib = lib
        ga = np.array([jm.point_words(g) for g in gens], np.uint64)
        self.h = C.c_void_p(lib.chk_vc_new(p(ga), G, N, EID_BITS, DEPTH, hash_leaves, 1))
        assert self.h
        s = np.zeros(10, np.uint64)
        lib.chk_vc_sizes(self.h, p(s))
        self.rows, self.inputs, self.vars, self.hashes, self.chunks, self.items, self.built_rows = (int(x) for x in s[:7])
        self.nnz = [int(x) for x in s[7:]]
        mats = []
        for k in range(3):
            rp = np.zeros(self.rows + 1, np.uint32); col = np.zeros(self.nnz[k], np.uint32); coef = np.zeros((self.nnz[k], 4), np.uint64)
            lib.chk_vc_csr(self.h, k, p(rp), p(col), p(coef))
            mats.append((rp, col, coef))
        self.mats = mats
        self.judge = vm.Judge(*mats)

    def block(self, b):
        first, count = C.c_uint32(0), C.c_uint32(0)
        assert self.lib.chk_vc_wires(self.h, b, C.byref(first), C.byref(count)) == 0
        return first.value, count.value

    def witness(self, eid, sk, index, vote, copath):
        out = np.zeros((self.vars, 4), np.uint64); leaf = np.zeros(4, np.uint64)
        cp = np.array([jm.words(c) for c in copath] + [[0, 0, 0, 0]], np.uint64)
        assert self.lib.chk_vc_witness(self.h, p(np.array(jm.message_words(eid), np.uint64)), p(np.array(jm.words(sk), np.uint64)), index, vote, p(cp), p(out), p(leaf)) == 0
        return out, vm.from_words(leaf)

    def first_bad_row(self, wit):
        bad = C.c_uint64(0)
        first = self.lib.chk_vc_first_bad_row(self.h, p(np.ascontiguousarray(wit)), C.byref(bad))
        return first, bad.value

    def both_judges_refuse(self, wit):
        first, bad = self.first_bad_row(wit)
        rows = self.judge.failing_rows(vm.witness_ints(wit))
        assert (first < self.rows) == bool(rows) and bad == len(rows) and (not rows or rows[0] == first)
        return bool(rows)

    def free(self):
        self.lib.chk_vc_free(self.h)


@pytest.fixture(scope="module", params=[1, 0], ids=["hashed_leaves", "plain_leaves"])
def election(request, lib, gens, table):
    """a circuit, four voters in a tree of depth 2, an eid, and every voter's witness (built once)"""
    hash_leaves = request.param
    circ = Circuit(lib, gens, hash_leaves)
    rng = random.Random(31 + hash_leaves)
    sks = [rng.getrandbits(255) for _ in range(4)]
    eid = [rng.getrandbits(1) for _ in range(EID_BITS)]
    levels = table.tree([vm.public_key(table, sk) for sk in sks], DEPTH, bool(hash_leaves))
    wits = []
    for x, sk in enumerate(sks):
        w, leaf = circ.witness(eid, sk, x, x % N, jm.copath(levels, x))
        assert leaf == levels[0][x]
        wits.append(w)
    yield circ, sks, eid, levels, wits
    circ.free()


def test_counts_equal_the_layout_functions_totals(election):
    circ = election[0]
    assert circ.built_rows == circ.rows and circ.lib.chk_vc_columns_ok(circ.h) == 1
    hashes = DEPTH + 2 + (1 if circ.hashes == DEPTH + 3 else 0)
    assert circ.hashes == hashes
    chunks = 85 * (hashes - DEPTH - 1) + 170 * DEPTH + (EID_BITS + 255 + 2) // 3
    assert circ.chunks == chunks
    assert circ.inputs == N + 1 + 2 + 2
    for rp, col, coef in circ.mats:
        assert rp[0] == 0 and rp[-1] == len(col) and (np.diff(rp.astype(np.int64)) >= 0).all()
        assert (col <= circ.vars).all()
        for r in range(circ.rows):
            row = col[rp[r]:rp[r + 1]]
            assert (np.diff(row.astype(np.int64)) > 0).all()
    # the named blocks lie inside the witness, the public ones first and in the reference's order
    firsts = [circ.block(b) for b in range(10)]
    assert [f for f, _ in firsts[:4]] == [0, N, N + 1, N + 3] and [c for _, c in firsts] == [N, 1, 2, 2, EID_BITS, 255, DEPTH, 255 * DEPTH, 255, 255]
    assert all(f + c <= circ.vars for f, c in firsts)


def test_every_voters_witness_satisfies_every_row(election):
    circ, _, _, _, wits = election
    for w in wits:
        assert circ.first_bad_row(w) == (circ.rows, 0)
        assert circ.judge.satisfied(vm.witness_ints(w))


def test_public_inputs_are_the_protocols(election, table):
    circ, sks, eid, levels, wits = election
    for x, (sk, w) in enumerate(zip(sks, wits)):
        assert vm.witness_ints(w[:circ.inputs]) == vm.public_inputs(table, N, eid, sk, x % N, levels[-1][0])
        sn_first, _ = circ.block(SN_BITS)
        sn = vm.serial_number(table, eid, sk)
        assert vm.witness_ints(w[sn_first:sn_first + 255]) == jm.bits_of(sn, 255)


def flip(w, at):
    out = w.copy()
    out[at, 0] ^= np.uint64(1)
    return out


def test_tampered_witnesses_are_refused(election):
    circ, _, _, _, wits = election
    w = wits[1]
    first = {b: circ.block(b)[0] for b in range(10)}
    cases = {"sn_packed": flip(w, first[SN_PACKED]), "rt_packed": flip(w, first[RT_PACKED]), "address": flip(w, first[ADDRESS] + 1), "sk": flip(w, first[SK] + 7),
             "copath": flip(w, first[COPATH] + 300), "eid_packed": flip(w, first[EID_PACKED])}
    two_hot = w.copy(); two_hot[first[M] + 2, 0] = 1
    none_hot = w.copy(); none_hot[first[M]:first[M] + N] = 0
    sn_bit = flip(w, first[SN_BITS] + 3)
    sn_bit[first[SN_PACKED]] = np.array(jm.words(vm.from_words(w[first[SN_PACKED]]) ^ 8), np.uint64)
    cases.update(two_hot=two_hot, none_hot=none_hot, sn_bit=sn_bit)
    assert circ.both_judges_refuse(w) is False
    for name, bad in cases.items():
        assert circ.both_judges_refuse(bad), name


def test_a_digest_has_one_bit_pattern(election, table, lib, gens):
    """a voter whose sn digest u is below 2^255 - r: SN_BITS = bits(u + r) with the consistent packing satisfies everything but the
    strict comparison"""
    circ, _, eid, levels, _ = election
    rng = random.Random(77)
    room = (1 << 255) - jm.R
    while True:
        sk = rng.getrandbits(255)
        u = vm.serial_number(table, eid, sk)
        if u < room:
            break
    # the host path proves membership in whatever tree the copath leads to: this witness is satisfied as it stands
    w, _ = circ.witness(eid, sk, 0, 0, jm.copath(levels, 0))
    before = set(circ.judge.failing_rows(vm.witness_ints(w)))
    assert not before
    first, _ = circ.block(SN_BITS)
    packed, _ = circ.block(SN_PACKED)
    alias = w.copy()
    bits = jm.bits_of(u + jm.R, 255)
    for i, b in enumerate(bits):
        alias[first + i] = [b, 0, 0, 0]
    lo, hi = vm.pack(bits)
    alias[packed] = np.array(jm.words(lo), np.uint64); alias[packed + 1] = np.array(jm.words(hi), np.uint64)
    after = set(circ.judge.failing_rows(vm.witness_ints(alias)))
    assert after, "the aliased digest satisfies the system"
    assert circ.first_bad_row(alias)[0] == min(after)


def test_stand_alone_program_under_sanitizers(tmp_path):
    """vote_circuit_check.cpp with its own main under AddressSanitizer and UBSan: no code loaded into python"""
    exe = str(tmp_path / "vote_circuit_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DVOTE_CIRCUIT_CHECK_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "vote_circuit_check: ok" in r.stdout, r.stdout + r.stderr
