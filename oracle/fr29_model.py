"""Exact limb-level model of the 9 x 29-bit lazy Fr arithmetic the NTT butterflies run on (vote_saver_protocol_amd/csrc/fr29.h,
k_ntt29_pass in ntt.hip), with the constants parsed from the generated header, and a worst-case propagation (value bound and per-limb
bound) through the butterflies.  Every routine raises Bound where the kernel's arithmetic would silently go wrong: a 32-bit limb that
wraps in either direction, a subtrahend that the redundant constant does not dominate, a product operand at or above 2^261.
tests/test_fr29_bounds.py drives it on the CPU; tests/test_gpu_ntt_structured.py uses it to craft inputs for the kernels."""
import os
import re

import bls12_381 as o

R = o.R
W, N = 29, 9
MASK = (1 << W) - 1
RP = 1 << (W * N)                      # R' = 2^261
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vote_saver_protocol_amd", "csrc", "mont_asm_gfx950.h")


def _consts():
    text = open(HEADER).read()
    return {name: [int(x.strip().rstrip("u"), 16) for x in body.split(",")]
            for name, body in re.findall(r"static constexpr uint32_t (FR29_\w+)\[9\] = \{([^}]*)\};", text)}


K = _consts()
RL, K2, K4 = K["FR29_R"], K["FR29_K2_L1"], K["FR29_K4_L1"]
ONE_PLAIN = [1] + [0] * (N - 1)        # the integer one: the fused load's second product only divides by 2^261


def val(l):
    return sum(x << (W * i) for i, x in enumerate(l))


def tight(v):
    assert 0 <= v < 1 << (W * (N - 1) + 32)
    return [(v >> (W * i)) & MASK for i in range(N - 1)] + [v >> (W * (N - 1))]


class Bound(AssertionError):
    pass


def need(c, msg):
    if not c:
        raise Bound(msg)


def mm29(a, b):
    for x in (a, b):
        need(all(0 <= t < 1 << 32 for t in x), "operand limb outside 32 bits")
    need(val(a) < RP and val(b) < RP, "operand not below 2^261")
    m, r, acc = [0] * N, [0] * N, 0
    for k in range(2 * N - 1):
        for i in range(max(0, k - N + 1), min(k, N - 1) + 1):
            acc += a[i] * b[k - i]
        for i in (range(0, k) if k < N else range(k - N + 1, N)):
            acc += m[i] * RL[k - i]
        if k < N:
            m[k] = ((-acc) & 0xFFFFFFFF) & MASK                             # v_sub_u32 tmp, 0, lo ; v_and_b32
            acc += m[k] * RL[0]
            need(acc & MASK == 0, "Montgomery column not cleared")
        else:
            r[k - N] = acc & MASK
        need(acc < 1 << 64, "column %d overflows the 64-bit accumulator" % k)
        acc >>= W
    need(acc < 1 << 32, "top limb overflows")
    r[N - 1] = acc
    need(val(r) * RP == val(a) * val(b) + val(m) * R, "not (a b + m r) / R'")
    need(val(r) < val(a) * val(b) // RP + R + 1 and all(x <= MASK for x in r[:-1]), "output not tight / above a b / R' + r")
    return r


def add29(a, b):
    r = [x + y for x, y in zip(a, b)]
    need(all(t < 1 << 32 for t in r), "sum wraps")
    return r


def sub29(a, b, k=K2):
    """a + k - b limb by limb; k is the redundant 2r (sub29) or 4r (sub29k4: the first stage of a fused load)"""
    name = "2r" if k is K2 else "4r"
    r = []
    for i in range(N):
        need(a[i] + k[i] < 1 << 32, "a + %s wraps" % name)
        need(a[i] + k[i] - b[i] >= 0, "a + %s - b borrows in limb %d" % (name, i))
        r.append(a[i] + k[i] - b[i])
    return r


def norm29(a):
    r, c = [], 0
    for i in range(N - 1):
        t = a[i] + c
        need(t < 1 << 32, "carry pass wraps")
        r.append(t & MASK); c = t >> W
    need(a[N - 1] + c < 1 << 32, "carry pass wraps the top limb")
    return r + [a[N - 1] + c]


def csub29(v):
    need(val(v) < 2 * R, "conditional subtraction of a value >= 2r")
    return tight(val(v) - R) if val(v) >= R else list(v)


def tw(x):
    return tight(x * RP % R)


def fused_load(a, b, c):
    """the first pass's fused load from canonical a, b, c: (a b - c) / 2^261 as a lazy value in (r, 3.02 r) -- NOT a product output"""
    return norm29(sub29(mm29(tight(a), tight(b)), mm29(tight(c), ONE_PLAIN)))


def radix4(x, w1, w2, w3, s_zero=False, k_first=K2):
    """one radix-4 step.  s_zero: the transform's first stage -- its twiddle is one, so x1 and x3 enter the subtractions as they were
    loaded, against k_first (the kernel: 2r for a plain or premultiplied load, 4r for the fused load)"""
    x0, x1, x2, x3 = x
    if not s_zero:
        x1, x3 = mm29(x1, w1), mm29(x3, w1)
        k_first = K2
    a0, a1, a2, a3 = add29(x0, x1), sub29(x0, x1, k_first), add29(x2, x3), sub29(x2, x3, k_first)
    a2, a3 = mm29(a2, w2), mm29(a3, w3)
    return [norm29(add29(a0, a2)), norm29(add29(a1, a3)), norm29(sub29(a0, a2)), norm29(sub29(a1, a3))]


def brev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else i


def model_ntt(vals, log_n, omega=None, k_first=K2, scale=None, loaded=False):
    """radix-2 decimation in time exactly as k_ntt29_pass steps it (an odd stage count starts with one radix-2 stage, then radix-4
    steps), one 'pass' over the whole array, values lazy throughout, canonical at the end through the product with `scale` (None: the
    Montgomery one).  vals: canonical integers in natural order, or -- loaded=True -- the limb vectors the first pass's load produced,
    still in natural order (position i of the tile takes entry brev(i)).  k_first: the constant the first stage subtracts against."""
    n = 1 << log_n
    omega = o.fr_root_of_unity(log_n) if omega is None else omega
    a = [vals[brev(i, log_n)] for i in range(n)]
    a = [list(v) for v in a] if loaded else [tight(v) for v in a]
    t = 0
    if log_n & 1:
        for q in range(n // 2):
            u, v = a[2 * q], a[2 * q + 1]
            a[2 * q], a[2 * q + 1] = norm29(add29(u, v)), norm29(sub29(u, v, k_first))
        t = 1
    while t < log_n:
        h = 1 << t
        for q in range(n // 4):
            mid_lo = q & (h - 1)
            mid0 = ((q >> t) << (t + 2)) | mid_lo
            e = [mid0, mid0 + h, mid0 + 2 * h, mid0 + 3 * h]
            w1 = tw(pow(omega, mid_lo << (log_n - 1 - t), R))
            w2 = tw(pow(omega, mid_lo << (log_n - 2 - t), R))
            w3 = tw(pow(omega, (mid_lo + h) << (log_n - 2 - t), R))
            out = radix4([a[i] for i in e], w1, w2, w3, s_zero=(t == 0), k_first=k_first)
            for i, v in zip(e, out):
                a[i] = v
        t += 2
    worst = max(val(v) for v in a)
    m = K["FR29_ONE"] if scale is None else tw(scale)
    return [val(csub29(mm29(v, m))) for v in a], worst


def first_stage_sources(log_n):
    """natural-order input indices that the first stage combines, as model_ntt loads them: quadruples (x0, x1, x2, x3) of the radix-4
    groups; for an odd stage count the radix-2 stage takes (x0, x1) and (x2, x3) of the same quadruples as its (u, v)"""
    return [tuple(brev(4 * q + j, log_n) for j in range(4)) for q in range(1 << (log_n - 2))]


# ------------------------------------------------------------------------------------------------ extreme fused triples
LOW_TRIPLE = (0, 1, 71 * R - RP)        # 0 * 1 / R' + 2r - (r - 1): the lazy value r + 1, the bottom of the fused load's range


def high_triple(floor=3.0):
    """canonical (a, b, 0) whose fused value is above floor * r: a b = (1 + d) r mod 2^261 makes the reduction multiplier 2^261 - 1 - d,
    so the product is nearly a b / 2^261 + r; the zero c subtracts nothing from the 2r that sub29 lends.  Search over d and a near
    r - 1 for a cofactor b that is canonical (one in 70 is), checked with the model."""
    for j in range(400):
        a = R - 2 - 2 * (j // 8)                                             # odd: invertible mod 2^261
        b = R * (1 + j % 8) * pow(a, -1, RP) % RP
        if b < R and val(fused_load(a, b, 0)) >= floor * R:
            return (a, b, 0)
    raise AssertionError("no extreme triple found")


# ------------------------------------------------------------------------------------------------ worst-case propagation
class B:
    def __init__(self, v, l):
        self.v, self.l = int(v), list(l)          # value < v, limb i < l[i]

    @staticmethod
    def tight(v):
        v = int(v)
        return B(v, [1 << W] * (N - 1) + [(v >> (W * (N - 1))) + 1])


def b_mul(a, b):
    worst, carry = 0, 0
    for k in range(2 * N - 1):
        col = carry
        for i in range(max(0, k - N + 1), min(k, N - 1) + 1):
            col += (a.l[i] - 1) * (b.l[k - i] - 1)
        for i in (range(0, k + 1) if k < N else range(k - N + 1, N)):
            col += MASK * RL[k - i]
        worst = max(worst, col); carry = col >> W
    need(worst < 1 << 64, "worst-case column sum reaches 2^64")
    need(a.v <= RP and b.v <= RP, "product operand may reach 2^261")
    return B.tight(a.v * b.v // RP + R + 1)


def b_add(a, b):
    l = [x + y - 1 for x, y in zip(a.l, b.l)]
    need(all(x <= 1 << 32 for x in l), "sum may wrap")
    return B(a.v + b.v, l)


def b_sub(a, b, k=K2):
    name = "2r" if k is K2 else "4r"
    need(all(k[i] >= b.l[i] - 1 for i in range(N)), "%s does not dominate the subtrahend's limbs" % name)
    need(all(a.l[i] - 1 + k[i] < 1 << 32 for i in range(N)), "a + %s may wrap" % name)
    return B(a.v + val(k), [a.l[i] + k[i] for i in range(N)])


def b_norm(a):
    need(all(x <= (1 << 32) - 8 for x in a.l), "carry pass may wrap")
    return B.tight(a.v)


def b_radix4(V, w, raw=False, k_first=K2):
    """bound of the outputs of one radix-4 step whose inputs are below V.  raw: the transform's first stage (no first pair of products;
    the loaded values are the subtrahends, against k_first)"""
    if raw:
        x1 = V
    else:
        x1 = b_mul(V, w); need(x1.v < 1.9 * R, "first product above 1.9 r"); k_first = K2
    a0, a1 = b_add(V, x1), b_sub(V, x1, k_first)
    p2, p3 = b_mul(a0, w), b_mul(a1, w); need(p3.v < 1.9 * R, "second product above 1.9 r")
    outs = [b_norm(b_add(a0, p2)), b_norm(b_add(a1, p3)), b_norm(b_sub(a0, p2)), b_norm(b_sub(a1, p3))]
    return B.tight(max(x.v for x in outs))


def b_transform(V, steps, odd=False, k_first=K2):
    """worst case of a whole transform from loaded values below V, stepped as the kernel steps it: the first stage takes the loaded
    values raw -- as one radix-2 stage (odd stage count; the radix-4 steps that follow all have their products) or inside the first
    radix-4 step -- then `steps` radix-4 steps in all; leaving the lazy domain needs the value below 2^261 and the last product below 2r.
    Returns the value bound after every stage, in units of r."""
    w = B.tight(R)                                                        # twiddles are canonical
    trace = []
    if odd:
        V = B.tight(max(b_norm(b_add(V, V)).v, b_norm(b_sub(V, V, k_first)).v)); trace.append(V.v / R)
    for step in range(steps):
        V = b_radix4(V, w, raw=(step == 0 and not odd), k_first=k_first); trace.append(V.v / R)
    need(V.v < RP, "value may reach 2^261")
    need(b_mul(V, w).v < 2 * R, "last product may reach 2r")
    return trace
