"""GPU tests of the voter registry (vsp_registry_*) against the big-integer model tests/jubjub_model.py, bit for bit: the tree at depths
0, 1, 2, 5 and 9 over full, nearly full, single-key and empty key lists with hashed and plain leaves -- root, rt scalars, every node of
every level, the blob, the copaths --; the variants (fused top levels, per-level launches, every lane-group size) against each other;
a root recomputed from a leaf and its copath by hash_batch alone; trees loaded from blobs, consistent and damaged; the link to the
ballot box's inputs; the argument errors."""
import ctypes as C
import random

import numpy as np
import pytest

import jubjub_model as jm
import vote_saver_protocol_amd as v

pytestmark = pytest.mark.gpu

G = 3
DEPTHS = [0, 1, 2, 5, 9]
ERR_ARG, ERR_UNSUPPORTED = -1, -4
NONE = 0xFFFFFFFFFFFFFFFF


def key_array(keys):
    return np.array([jm.words(k) for k in keys], np.uint64).reshape(-1, 4)


def as_ints(a):
    return [sum(int(x) << (64 * i) for i, x in enumerate(row)) for row in np.asarray(a).reshape(-1, 4)]


@pytest.fixture(scope="module")
def gens():
    return jm.generators(G)


@pytest.fixture(scope="module")
def model(gens):
    return jm.Table(gens)


@pytest.fixture(scope="module")
def ped(ctx, gens):
    h = v.Pedersen(ctx, np.array([jm.point_words(g) for g in gens], np.uint64))
    yield h
    h.free()


@pytest.fixture(scope="module")
def keys():
    rng = random.Random(31)
    return [rng.getrandbits(255) for _ in range(1 << max(DEPTHS))]


@pytest.fixture(scope="module")
def trees(model, keys):
    """the model's trees, each computed once: (depth, count, hash_leaves) -> levels"""
    cache = {}

    def get(depth, count, hash_leaves):
        k = (depth, count, bool(hash_leaves))
        if k not in cache:
            cache[k] = model.tree(keys[:count], depth, bool(hash_leaves))
        return cache[k]
    return get


@pytest.fixture
def options(ctx):
    yield ctx.set_option
    ctx.set_option("pedersen_lanes", 0)
    ctx.set_option("registry_fused_levels", 0)


def counts_of(depth):
    return sorted({1 << depth, (1 << depth) - 1, 1, 0})


@pytest.mark.parametrize("hash_leaves", [1, 0])
@pytest.mark.parametrize("depth", DEPTHS)
def test_build_against_the_model(ctx, ped, keys, trees, depth, hash_leaves):
    for count in counts_of(depth):
        levels = trees(depth, count, hash_leaves)
        with v.Registry.build(ctx, ped, key_array(keys[:count]), depth, hash_leaves=bool(hash_leaves)) as reg:
            assert reg.depth == depth and reg.device_bytes() >= 32 * ((2 << depth) - 1)
            root = levels[-1][0]
            assert as_ints(reg.root()) == [root]
            assert as_ints(reg.rt_scalars()) == jm.rt_scalars(root) == [root % (1 << 254), root >> 254]
            for l in range(depth + 1):
                assert as_ints(reg.nodes(l)) == levels[l], (depth, count, l)
            if depth >= 2:
                assert as_ints(reg.nodes(1, 1, 1)) == levels[1][1:2]
            assert reg.to_blob() == jm.tree_blob(levels)
            indices = list(range(1 << depth)) if depth <= 5 else [0, 1, (1 << depth) - 1, 77, 77]
            paths = reg.paths(indices)
            assert paths.shape == (len(indices), depth, 4)
            for row, x in zip(paths, indices):
                assert as_ints(row) == jm.copath(levels, x), (depth, count, x)


def test_variants_give_identical_trees(ctx, ped, keys, trees, options):
    """depth 9: no fused level, the top 3 and all 9 in the single-workgroup launch, and every lane-group size of the per-level
    launches -- one tree, the model's"""
    depth = 9
    want = jm.tree_blob(trees(depth, 1 << depth, 1))
    pks = key_array(keys[:1 << depth])
    for fused, lanes in ((-1, 0), (3, 0), (9, 0), (-1, 1), (-1, 4), (3, 16), (-1, 64), (9, 1), (0, 0)):
        options("registry_fused_levels", fused)
        options("pedersen_lanes", lanes)
        with v.Registry.build(ctx, ped, pks, depth) as reg:
            assert reg.to_blob() == want, (fused, lanes)
    assert ctx.stat("registry_build_ms") > 0


def test_root_from_a_leaf_and_its_copath_by_hash_batch_alone(ctx, ped, keys):
    depth = 9
    with v.Registry.build(ctx, ped, key_array(keys[:1 << depth]), depth) as reg:
        root = reg.root()
        for x in (0, 1, 300, (1 << depth) - 1):
            path = reg.paths([x])[0]
            node = v.pedersen_hash_batch(ctx, ped, key_array([keys[x]]), 255)[0]
            assert np.array_equal(node, reg.nodes(0, x, 1)[0])
            for l in range(depth):
                pair = (path[l], node) if (x >> l) & 1 else (node, path[l])
                bits = jm.bits_of(as_ints(pair[0])[0], 255) + jm.bits_of(as_ints(pair[1])[0], 255)
                node = v.pedersen_hash_batch(ctx, ped, np.array([jm.message_words(bits)], np.uint64), 510)[0]
            assert np.array_equal(node, root), x
        assert ctx.stat("registry_paths_ms") > 0


def flip(blob, node, bit):
    b = bytearray(blob)
    b[32 * node + bit // 8] ^= 1 << (7 - bit % 8)
    return bytes(b)


@pytest.mark.parametrize("depth", [0, 2, 5, 9])
def test_from_blob_round_trip_and_damage(ctx, ped, keys, trees, depth, options):
    levels = trees(depth, 1 << depth, 1)
    blob = jm.tree_blob(levels)
    nodes = (2 << depth) - 1
    assert ctx.lib.vsp_registry_blob_size(depth) == len(blob) == 32 * nodes
    for lanes in (0, 1) if depth == 5 else (0,):
        options("pedersen_lanes", lanes)
        with v.Registry.from_blob(ctx, ped, blob, depth) as reg:
            assert reg.first_bad_node is None and reg.to_blob() == blob and as_ints(reg.root()) == levels[-1]
            if depth:
                assert as_ints(reg.paths([1])[0]) == jm.copath(levels, 1)
        if depth == 0:
            continue
        leaves = 1 << depth
        for leaf in (0, 3, leaves - 1):                              # one flipped bit in a leaf: the leaf's parent
            with v.Registry.from_blob(ctx, ped, flip(blob, leaf, 17), depth) as reg:
                assert reg.first_bad_node == leaves + leaf // 2
        with v.Registry.from_blob(ctx, ped, flip(blob, nodes - 1, 254), depth) as reg:      # one flipped bit in the root: the root
            assert reg.first_bad_node == nodes - 1
        with v.Registry.from_blob(ctx, ped, flip(flip(blob, nodes - 1, 0), 2, 100), depth) as reg:      # two damaged nodes: the lower index
            assert reg.first_bad_node == leaves + 1
        if depth >= 2:
            # an inner node differs from its children AND its parent from it: the inner node is the lower
            with v.Registry.from_blob(ctx, ped, flip(blob, leaves + 1, 5), depth) as reg:
                assert reg.first_bad_node == leaves + 1
        with v.Registry.from_blob(ctx, ped, flip(blob, 2, 100), depth, verify=False) as reg:
            assert reg.first_bad_node is None and reg.to_blob() == flip(blob, 2, 100)
    assert ctx.stat("registry_check_ms") > 0 or depth == 0


def test_from_blob_refuses_a_wrong_length_and_a_set_256th_bit(ctx, ped, trees):
    blob = jm.tree_blob(trees(2, 4, 1))
    for bad in (blob[:-1], blob + b"\0", blob[:-32], b""):
        with pytest.raises(v.VspError, match="vsp error -1"):
            v.Registry.from_blob(ctx, ped, bad, 2)
    for node in (0, 6):
        b = bytearray(blob); b[32 * node + 31] |= 1                  # bit 255 of a node
        with pytest.raises(v.VspError, match="256th bit"):
            v.Registry.from_blob(ctx, ped, bytes(b), 2, verify=bool(node))


def test_link_to_the_ballot_box_inputs(ctx, ped, keys):
    """rt and sn = H(eid | sk) as the circuit's public inputs: two scalars each, of 254 bits and 1 bit, canonical -- the shape and range
    of a BallotBox's FIXED values and serials (no election is run)"""
    below_r = lambda row: as_ints(row)[0] < jm.R
    with v.Registry.build(ctx, ped, key_array(keys[:32]), 5) as reg:
        rt = reg.rt_scalars()
    assert rt.shape == (2, 4) and rt.dtype == np.uint64 and all(below_r(s) for s in rt)
    assert as_ints(rt[0])[0] < 1 << 254 and as_ints(rt[1])[0] < 2
    rng = random.Random(33)
    eid = [rng.getrandbits(1) for _ in range(64)]
    messages = [eid + jm.bits_of(rng.getrandbits(255), 255) for _ in range(65)]
    sn = v.pedersen_hash_batch(ctx, ped, np.array([jm.message_words(m) for m in messages], np.uint64), 64 + 255)
    serials = v.digest_scalars(sn)
    assert serials.shape == (65, 2, 4) and serials.dtype == np.uint64
    for d, s in zip(as_ints(sn), serials):
        assert as_ints(s) == jm.rt_scalars(d) and all(below_r(x) for x in s)
    assert len({tuple(as_ints(s)) for s in serials}) == 65


def test_argument_errors(ctx, ped, gens, keys):
    lib = ctx.lib
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    pks = key_array(keys[:4])
    h = C.c_void_p(None)
    assert lib.vsp_registry_build(ctx.h, ped.h, None, 0, 2, 1, C.byref(h)) == ERR_ARG and not h.value      # a null pointer even with count 0
    assert lib.vsp_registry_build(ctx.h, None, p(pks), 4, 2, 1, C.byref(h)) == ERR_ARG
    assert lib.vsp_registry_build(ctx.h, ped.h, p(pks), 4, 2, 1, None) == ERR_ARG
    assert lib.vsp_registry_build(None, ped.h, p(pks), 4, 2, 1, C.byref(h)) == ERR_ARG
    assert lib.vsp_registry_build(ctx.h, ped.h, p(pks), 4, 25, 1, C.byref(h)) == ERR_UNSUPPORTED and not h.value
    assert lib.vsp_registry_build(ctx.h, ped.h, p(pks), 4, 1, 1, C.byref(h)) == ERR_ARG                   # more keys than leaves
    high = pks.copy(); high[2, 3] |= np.uint64(1 << 63)
    assert lib.vsp_registry_build(ctx.h, ped.h, p(high), 4, 2, 1, C.byref(h)) == ERR_ARG and "key 2" in ctx.last_error()
    with v.Pedersen(ctx, np.array([jm.point_words(g) for g in gens[:2]], np.uint64)) as two:              # g < 3
        assert lib.vsp_registry_build(ctx.h, two.h, p(pks), 4, 2, 1, C.byref(h)) == ERR_ARG and "3 generators" in ctx.last_error()
        assert lib.vsp_registry_from_blob(ctx.h, two.h, p(np.zeros(32 * 7, np.uint8)), 32 * 7, 2, 1, C.byref(h), None) == ERR_ARG
    assert lib.vsp_registry_from_blob(ctx.h, ped.h, None, 32 * 7, 2, 1, C.byref(h), None) == ERR_ARG
    assert lib.vsp_registry_from_blob(ctx.h, ped.h, p(np.zeros(32, np.uint8)), 32, 25, 1, C.byref(h), None) == ERR_UNSUPPORTED
    assert lib.vsp_registry_blob_size(25) == 0 and lib.vsp_registry_blob_size(20) == 32 * ((1 << 21) - 1)
    with v.Registry.build(ctx, ped, pks, 2) as reg:
        out = np.zeros((4, 2, 4), np.uint64)
        idx = np.array([0, 3, 4], np.uint64)
        assert lib.vsp_registry_paths(ctx.h, reg.h, p(idx), 2, p(out)) == 0
        assert lib.vsp_registry_paths(ctx.h, reg.h, p(idx), 3, p(out)) == ERR_ARG and "index 2" in ctx.last_error()      # index 2^D
        assert lib.vsp_registry_paths(ctx.h, reg.h, None, 0, p(out)) == ERR_ARG
        assert lib.vsp_registry_paths(ctx.h, reg.h, p(idx), 0, None) == ERR_ARG
        assert lib.vsp_registry_paths(ctx.h, reg.h, p(idx), 0, p(out)) == 0
        assert lib.vsp_registry_paths(ctx.h, None, p(idx), 1, p(out)) == ERR_ARG
        assert lib.vsp_registry_nodes(ctx.h, reg.h, 3, 0, 1, p(out)) == ERR_ARG                            # a level above the root
        assert lib.vsp_registry_nodes(ctx.h, reg.h, 1, 1, 2, p(out)) == ERR_ARG                            # a range outside the level
        assert lib.vsp_registry_nodes(ctx.h, reg.h, 1, 2, 0, p(out)) == 0
        assert lib.vsp_registry_nodes(ctx.h, reg.h, 0, 0, 4, None) == ERR_ARG
        assert lib.vsp_registry_root(ctx.h, reg.h, None, None) == ERR_ARG
        assert lib.vsp_registry_to_blob(ctx.h, reg.h, None) == ERR_ARG
        assert lib.vsp_registry_root(ctx.h, reg.h, p(out), None) == 0                                     # usable after every refusal
    assert lib.vsp_registry_depth(None) == 0 and lib.vsp_registry_device_bytes(None) == 0
