"""GPU: the NTT and witness_map on STRUCTURED and worst-case inputs -- what uniformly random field elements almost never produce:
outputs that are exact multiples of r (the conditional subtraction's boundary), maximal lazy growth through every pass, and the two
ends of the value range of witness_map's fused load (tests/test_fr29_bounds.py holds the CPU model of the same discipline).

 a. transforms with closed forms: the expected values come from Python big integers (geometric sums, single characters), the C oracle
    is a second witness; all four modes, both butterfly kernels (9 x 29-bit lazy and 8 x 32-bit);
 b. witness_map fed with coset evaluations crafted from the extreme fused triples of oracle/fr29_model.py, in every low / high pattern
    over a first-stage butterfly: the fused batched path, the sequence (witness_map_batched = 0) and the 8 x 32-bit kernel must all
    give the H of plain integers.  (The 29-bit first stage before sub29k4 subtracted these values against 2r and returned a wrong H.)

Sizes: with NTT_TILE_LOG = 11 and NTT_MAX_STAGES = 8, ntt_plan (ntt.hip) gives, as stages per pass,
    2^2: 2    2^3: 3    2^4: 4    2^11: 11 (one pass; even, odd, even, odd stage count)
    2^12: 6 + 6    2^13: 7 + 6    2^16: 8 + 8 (the real circuit's size)    2^17: 6 + 6 + 5
so every plan shape is met with an odd and an even first pass (an odd count starts with the radix-2 stage)."""
import functools

import numpy as np
import pytest

import bls12_381 as o
import fr29_model as fm
from conftest import L

import vote_saver_protocol_amd as v

pytestmark = pytest.mark.gpu
R = o.R
G = 7
G7 = L(G, 4)
PLANS = {2: [2], 3: [3], 4: [4], 11: [11], 12: [6, 6], 13: [7, 6], 16: [8, 8], 17: [6, 6, 5]}
MODES = {"fft": (False, None), "ifft": (True, None), "coset": (False, G7), "icoset": (True, G7)}


def ntt_plan(log_m, tile_log=11, max_stages=8):
    """ntt.hip ntt_plan: passes of at most max_stages stages, as even as the count allows, a stage traded between two odd passes"""
    npass = 1 if log_m <= tile_log else (log_m + max_stages - 1) // max_stages
    st = [log_m // npass + (1 if i < log_m % npass else 0) for i in range(npass)]
    for i in range(npass - 1):
        if st[i] & 1:
            for k in range(i + 1, npass):
                if st[k] & 1 and st[i] < max_stages and st[k] > 1:
                    st[i] += 1; st[k] -= 1
                    break
    return st


def to_arr(vals):
    return np.frombuffer(b"".join(x.to_bytes(32, "little") for x in vals), dtype=np.uint64).reshape(-1, 4).copy()


def canonical(arr):
    lt, eq = np.zeros(arr.shape[0], bool), np.ones(arr.shape[0], bool)
    for k in (3, 2, 1, 0):
        rk = np.uint64((R >> (64 * k)) & 0xFFFFFFFFFFFFFFFF)
        lt |= eq & (arr[:, k] < rk); eq &= arr[:, k] == rk
    return bool(lt.all())


def powers(x, n):
    out, acc = [], 1
    for _ in range(n):
        out.append(acc); acc = acc * x % R
    return out


def batch_inv(xs):
    pre, acc = [], 1
    for x in xs:
        pre.append(acc); acc = acc * x % R
    inv, out = pow(acc, -1, R), [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        out[i] = inv * pre[i] % R; inv = inv * xs[i] % R
    return out


@functools.lru_cache(maxsize=2)
def tables(log_m):
    """omega^j, g^j, g^-j and the coset transform of the constant one, D[j] = sum_i (g omega^j)^i = (g^m - 1) / (g omega^j - 1)"""
    m = 1 << log_m
    Wp = powers(o.fr_root_of_unity(log_m), m)
    gm1 = (pow(G, m, R) - 1) % R
    D = [gm1 * x % R for x in batch_inv([(G * w - 1) % R for w in Wp])]
    return Wp, powers(G, m), powers(pow(G, -1, R), m), D


def expect(log_m, form, mode):
    """closed forms.  form ("chars", [(c, k), ...]): a_i = sum c omega^(-k i) -- a constant is k = 0; ("deltas", [(c, k), ...]): a = sum c e_k"""
    m = 1 << log_m
    Wp, GP, GI, D = tables(log_m)
    minv = pow(m, -1, R)
    kind, terms = form
    scale = lambda xs, c: xs if c == 1 else [c * x % R for x in xs]
    if kind == "chars" and mode != "coset":
        out = [0] * m
        for c, k in terms:
            if mode == "fft":                          # sum_i omega^(i (j - k)) = m at j = k, 0 elsewhere
                out[k] = (out[k] + m * c) % R
            else:                                      # one at j = -k; the inverse coset transform multiplies output j by g^-j
                j = (-k) % m
                out[j] = (out[j] + c * (GI[j] if mode == "icoset" else 1)) % R
        return out
    parts = []
    for c, k in terms:
        if kind == "chars":                            # sum_i (g omega^(j - k))^i, the geometric sum: D[j - k]
            parts.append(scale(D[m - k:] + D[:m - k], c))
        elif mode in ("fft", "coset"):                 # c g^k omega^(j k)
            parts.append(scale([Wp[j * k % m] for j in range(m)], c * (GP[k] if mode == "coset" else 1) % R))
        else:                                          # c / m omega^(-j k)
            parts.append(scale([Wp[-j * k % m] for j in range(m)], c * minv % R))
    out = parts[0] if len(parts) == 1 else [sum(xs) % R for xs in zip(*parts)] if parts else [0] * m
    if kind == "deltas" and mode == "icoset":
        out = [x * gi % R for x, gi in zip(out, GI)]
    return out


@functools.lru_cache(maxsize=1)
def structured_inputs(log_m):
    """(name, input values, closed form or None)"""
    m = 1 << log_m
    Wp = tables(log_m)[0]
    half = (R + 1) // 2                                   # 1 / 2
    cases = [("zero", [0] * m, ("chars", []))]
    for c in (1, R - 1, (R - 1) // 2):                    # all r - 1: maximal lazy growth; m - 1 outputs are multiples of r
        cases.append(("constant %x" % c, [c] * m, ("chars", [(c, 0)])))
    for c, k in zip((1, R - 1, (R - 1) // 2, (1 << 254) - 1), (0, 1, m // 2, m - 1)):
        cases.append(("delta at %d" % k, [c if i == k else 0 for i in range(m)], ("deltas", [(c, k)])))
    for k in (1, m - 1):
        cases.append(("character %d" % k, [Wp[-k * i % m] for i in range(m)], ("chars", [(1, k)])))
    # 0, r - 1, 0, r - 1, ...: -1/2 + (-1)^i / 2, the characters 0 and m / 2
    cases.append(("alternating", [0, R - 1] * (m // 2), ("chars", [(R - half, 0), (half, m // 2)])))
    rng = np.random.default_rng(1000 + log_m)
    ones = sorted(set(np.flatnonzero(rng.random(m) < 0.1).tolist()) | {m - 1})
    sparse = [0] * m
    for i in ones:
        sparse[i] = 1
    # the shape of a real witness column; as a sum of deltas in big integers up to 2^11 (|ones| m products), the C oracle alone beyond
    cases.append(("sparse booleans", sparse, ("deltas", [(1, k) for k in ones]) if log_m <= 11 else None))
    return cases


@pytest.fixture(scope="module")
def paths():
    """a context per butterfly kernel: option ntt_fr29 = 1 (the default; the known-answer check must have passed) and 0"""
    c29, c32 = v.Context(0), v.Context(0)
    c32.set_option("ntt_fr29", 0)
    try:
        yield {1: c29, 0: c32}
    finally:
        c32.set_option("ntt_fr29", 1)
        c29.close(); c32.close()


def test_the_plans_this_file_is_sized_for():
    assert {lm: ntt_plan(lm) for lm in PLANS} == PLANS


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("log_m", sorted(PLANS))
def test_closed_form_transforms(paths, cref, log_m, mode):
    m = 1 << log_m
    inverse, coset = MODES[mode]
    doms = {f29: v.EvaluationDomain(c, m) for f29, c in paths.items()}
    try:
        for name, vals, form in structured_inputs(log_m):
            a = to_arr(vals)
            want = cref.ntt_fr(a, inverse=inverse, coset=coset)
            if form is not None:
                closed = to_arr(expect(log_m, form, mode))
                assert np.array_equal(want, closed), ("C oracle against the closed form", name, mode)
                want = closed
            if log_m <= 4:
                vin = [x * g % R for x, g in zip(vals, tables(log_m)[1])] if mode == "coset" else vals
                w = o.fr_root_of_unity(log_m)
                naive = o.dft_naive(vin, pow(w, -1, R) if inverse else w)
                if inverse:
                    naive = [x * pow(m, -1, R) * (tables(log_m)[2][j] if coset is not None else 1) % R for j, x in enumerate(naive)]
                assert np.array_equal(want, to_arr(naive)), ("the definition", name, mode)
            for f29, dom in doms.items():
                got = dom._run(a, inverse, coset)
                assert canonical(got), (name, mode, f29)
                assert np.array_equal(got, want), (name, mode, f29)
                assert paths[f29].stat("ntt_fr29") == f29 and paths[f29].stat("ntt_passes") == len(PLANS[log_m])
    finally:
        for d in doms.values():
            d.free()


# ------------------------------------------------------------------------------------------------ witness_map at the ends of the fused load
@functools.lru_cache(maxsize=1)
def extreme_triples():
    lo, hi = fm.LOW_TRIPLE, fm.high_triple(3.0)
    return lo, hi, fm.val(fm.fused_load(*lo)), fm.val(fm.fused_load(*hi))


def crafted_coset_evaluations(log_m, run):
    """a', b', c' on the coset: random canonical filler, and -- in the groups whose x0 is among the first or last 32 indices or a
    multiple of 61 -- the low / high triple in pattern (x0 index + run m / 4) mod 16, bit j deciding x_j.  The quadruples
    (x0, x1, x2, x3) come from the model's own load order; an odd first pass takes (x0, x1) and (x2, x3) as its radix-2 pairs."""
    m = 1 << log_m
    lo, hi, _, _ = extreme_triples()
    rng = np.random.default_rng(7000 + 100 * log_m + run)
    fill = rng.integers(0, 1 << 64, size=(3, m, 4), dtype=np.uint64)
    fill[:, :, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
    cols = [[int.from_bytes(row.tobytes(), "little") for row in fill[t]] for t in range(3)]
    patterns = set()
    for src in fm.first_stage_sources(log_m):
        i = src[0]
        assert src == (i, i + m // 2, i + m // 4, i + 3 * m // 4) and i < m // 4
        if i < 32 or i >= m // 4 - 32 or i % 61 == 0:
            pattern = (i + run * (m // 4)) % 16
            patterns.add(pattern)
            for j, pos in enumerate(src):
                for t in range(3):
                    cols[t][pos] = (hi if pattern >> j & 1 else lo)[t]
    return cols, patterns


@pytest.mark.parametrize("log_m", [2, 3, 4, 11, 12, 13, 16])
def test_witness_map_at_both_ends_of_the_fused_load(paths, cref, log_m):
    """the first stage of witness_map's last transform takes the fused values (a' b' - c') / 2^261 raw, as subtrahends: lazy values from
    r + 1 to above 3.0 r.  Inputs made so that the kernel's fused load sees exactly the crafted a', b', c': Az = NTT(icosetNTT(a'))."""
    lo, hi, vlo, vhi = extreme_triples()
    assert vlo <= 1.001 * R and vhi >= 3.0 * R
    m = 1 << log_m
    zinv = pow(pow(G, m, R) - 1, -1, R)
    seen = set()
    c29, c32 = paths[1], paths[0]
    for run in range(max(1, 16 // (m // 4))):
        (ap, bp, cp), patterns = crafted_coset_evaluations(log_m, run)
        seen |= patterns
        Az, Bz, Cz = (cref.ntt_fr(cref.ntt_fr(to_arr(x), inverse=True, coset=G7)) for x in (ap, bp, cp))
        q = [(a * b - c) * zinv % R for a, b, c in zip(ap, bp, cp)]
        want = cref.ntt_fr(to_arr(q), inverse=True, coset=G7)
        if log_m <= 4:                                    # the definition in big integers: h_j = g^-j / m sum_i q_i omega^(-i j)
            naive = o.dft_naive(q, pow(o.fr_root_of_unity(log_m), -1, R))
            assert np.array_equal(want, to_arr([x * pow(m, -1, R) * pow(G, -j, R) % R for j, x in enumerate(naive)]))
        got = v.witness_map_h(c29, Az, Bz, Cz)
        assert c29.stat("ntt_fused_load") == 1 and c29.stat("ntt_fr29") == 1 and c29.stat("ntt_passes") == len(PLANS[log_m])
        assert np.array_equal(got, want), "fused, batched path"
        c29.set_option("witness_map_batched", 0)
        try:
            got = v.witness_map_h(c29, Az, Bz, Cz)
            assert c29.stat("ntt_fused_load") == 0 and c29.stat("ntt_fr29") == 1
        finally:
            c29.set_option("witness_map_batched", 1)
        assert np.array_equal(got, want), "sequence of transforms, 29-bit butterflies"
        got = v.witness_map_h(c32, Az, Bz, Cz)
        assert c32.stat("ntt_fused_load") == 0 and c32.stat("ntt_fr29") == 0
        assert np.array_equal(got, want), "8 x 32-bit butterflies"
    assert len(seen) == 16
