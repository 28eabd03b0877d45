"""CPU build of the LDS counting sort's block mapping and round count (vote_saver_protocol_amd/csrc/lds_sort_map.h, the header that
k_count_lds, k_scatter_lds and their host code share): tests/cpu_build/lds_sort_map_check.cpp is a program of its own, built by g++ with
AddressSanitizer and UBSan.  For every W in 1..64 and every chunk count 1..256 it checks both mappings.  The even one (a single
pass, and every sort the library chooses rounds for by itself): block ids 0 .. W chunks - 1 map one-to-one onto the (window, chunk)
pairs, and for W a multiple of 8 all chunks of a window share block % 8.  The labelled one (rounds forced for any other W): the
blocks which own something map one-to-one onto the pairs and all chunks of a window share block % 8.

In the labelled mapping the block ids are 0 .. lds_sort_grid(W, chunks, True) - 1, not 0 .. W chunks - 1: whole windows on one label
cannot use every block id unless W is a multiple of 8 (W = 1, two chunks: blocks 0 and 1 carry different labels), so for any other W the
grid is rounded up and the surplus blocks own nothing.  The program checks that a multiple of 8 has no such block and that the two
mappings are then the same.  No GPU, no HIP."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpu_build", "lds_sort_map_check.cpp")


def test_block_mapping_and_round_count(tmp_path):
    exe = str(tmp_path / "lds_sort_map_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "lds_sort_map_check: ok" in r.stdout, r.stdout + r.stderr
