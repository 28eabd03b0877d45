"""CPU test of the drop-in boundary for the voting circuit: libvsp_hip.so loads without a GPU, exports every vsp_vote_* symbol that
include/vsp.h declares, each has a ctypes prototype of the declared arity, and the handle-free calls refuse null handles."""
import os
import re

import vote_saver_protocol_amd as v
from conftest import ROOT
from vote_saver_protocol_amd import _lib

EXPECTED = ["vsp_vote_cast_batch", "vsp_vote_circuit_create", "vsp_vote_circuit_csr", "vsp_vote_circuit_free", "vsp_vote_circuit_r1cs", "vsp_vote_circuit_sizes",
            "vsp_vote_circuit_wires", "vsp_vote_witness_batch", "vsp_vote_witness_host"]


def declarations():
    text = open(os.path.join(ROOT, "include", "vsp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {name: args for name, args in re.findall(r"\b(vsp_vote_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}


def test_vote_circuit_symbols_are_exported_and_prototyped():
    lib = v.load()
    decl = declarations()
    assert sorted(decl) == EXPECTED
    for name, args in decl.items():
        assert hasattr(lib, name), f"{name} declared in include/vsp.h but not exported"
        assert name in _lib.PROTOTYPES, f"{name} has no ctypes prototype"
        assert len(_lib.PROTOTYPES[name][1]) == len(args.split(",")), f"{name}: the prototype's arity is not the header's"


def test_block_names_of_the_python_layer_follow_the_header():
    text = open(os.path.join(ROOT, "include", "vsp.h")).read()
    values = {name: int(val) for name, val in re.findall(r"VSP_VOTE_([A-Z_]+) = (\d+)", text)}
    assert [values[b] for b in v.api.VoteCircuit.BLOCKS] == list(range(10))


def test_null_handles_are_refused_without_a_gpu():
    lib = v.load()
    assert lib.vsp_vote_circuit_r1cs(None) is None
    assert lib.vsp_vote_circuit_sizes(None, None, None, None, None) == -1
    assert lib.vsp_vote_circuit_csr(None, 0, None, None, None) == -1
    assert lib.vsp_vote_circuit_wires(None, 0, None, None) == -1
    assert lib.vsp_vote_witness_host(None, None, None, 0, 0, None, None, None) == -1
    assert lib.vsp_vote_witness_batch(None, None, None, None, None, None, None, 0, None, None) == -1
    lib.vsp_vote_circuit_free(None, None)
