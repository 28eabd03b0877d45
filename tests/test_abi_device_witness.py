"""CPU test of the drop-in boundary for the device witness source: every entry point that include/vsp.h declares for it is exported,
has a ctypes prototype of the declared arity, and refuses a null context without a GPU."""
import os
import re

import vote_saver_protocol_amd as v
from conftest import ROOT
from vote_saver_protocol_amd import _lib

EXPECTED = ["vsp_cast_batch_finish", "vsp_cast_batch_launch", "vsp_cast_witness_batch_device", "vsp_cast_witness_release", "vsp_groth16_prove_batch_device",
            "vsp_groth16_prove_batch_launch_device", "vsp_r1cs_check_batch_device", "vsp_saver_encrypt_batch_device", "vsp_saver_encrypt_batch_launch_device"]


def declarations():
    text = open(os.path.join(ROOT, "include", "vsp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {name: args for name, args in re.findall(r"\b(vsp_cast_[a-z0-9_]+|vsp_[a-z0-9_]+_device)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}


def test_device_witness_symbols_are_exported_and_prototyped():
    lib = v.load()
    decl = declarations()
    assert sorted(n for n in decl if n in EXPECTED) == EXPECTED
    for name in EXPECTED:
        assert hasattr(lib, name), f"{name} declared in include/vsp.h but not exported"
        assert len(_lib.PROTOTYPES[name][1]) == len(decl[name].split(",")), f"{name}: the prototype's arity is not the header's"


def test_a_null_context_is_refused_without_a_gpu():
    lib = v.load()
    for name in EXPECTED:
        args = [None if t is _lib._P else 0 for t in _lib.PROTOTYPES[name][1]]
        assert getattr(lib, name)(*args) == -1, name
