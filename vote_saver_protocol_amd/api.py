"""Host-side mirror of the reference's interface for the prover hot path, on top of the C ABI.

The reference exposes this path as C++ templates (absent crypto3 submodules):
    algebra::multiexp<multiexp_method_BDLO12>(bases_begin, bases_end, scalars_begin, scalars_end, chunks)
    algebra::multiexp_with_mixed_addition<...>(...)
    math::make_evaluation_domain<Fr>(m) -> evaluation_domain { m, fft, inverse_fft, ... }
    zk::snark::r1cs_gg_ppzksnark prover (reached from bin/cli/include/nil/vote_saver/common.hpp:1132-1135)
This module keeps the same names and argument meaning with numpy arrays of canonical little-endian
uint64 limbs (Fr: [n,4], G1 affine: [n,12], G2 affine: [n,24]; infinity = all zero).  Every call goes
through libvsp_hip.so; nothing here computes field or curve arithmetic on the CPU.
"""
import collections
import ctypes as C
import secrets

import numpy as np

from . import _lib


class VspError(RuntimeError):
    pass


class Unsatisfied(VspError):
    """VSP_ERR_UNSATISFIED (option "prove_check_witness"): a witness does not satisfy the constraint system.  code = -5; first_bad_row: the
    first failing constraint of a single proof; after a batch: status [K] (bit 1 = unsatisfied), first_bad_row [K] and results = the
    batch's (A, B, C, proofs), where the satisfied members' proofs are valid and the others' outputs all zero."""
    code = -5
    first_bad_row = None
    status = None
    results = None


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    if isinstance(a, int):
        return C.c_void_p(a)
    if hasattr(a, "data_ptr"):          # torch tensor (device or host memory)
        return C.c_void_p(a.data_ptr())
    raise TypeError(type(a))


def _u64(a, cols=None):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if cols is not None:
        a = a.reshape(-1, cols)
    return a


# per group: uint64 words of a canonical affine point and of a Jacobian record, and the suffix of the group's C entry points
_Group = collections.namedtuple("_Group", "affine jacobian suffix")
_GROUPS = {1: _Group(12, 18, "_g1"), 2: _Group(24, 36, "_g2")}


def _group(group):
    """the table row of `group`; every value other than 1 sizes as G2 (the library refuses a group it does not know)"""
    return _GROUPS[1] if group == 1 else _GROUPS[2]


class Context:
    """One GPU + one HIP stream + grow-only device workspaces (vsp_ctx)."""

    def __init__(self, device=0):
        self.lib = _lib.load()
        self.h = self.lib.vsp_create(int(device))
        if not self.h:
            raise VspError(f"vsp_create({device}) failed: no such HIP device (this path has no CPU fallback)")
        self.device = device
        self.options = {}                   # what set_option has set (the library has no getter): lets a caller put a value back

    def close(self):
        if self.h:
            self.lib.vsp_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc == Unsatisfied.code:
            raise Unsatisfied(f"vsp error {rc}: {self.lib.vsp_last_error(self.h).decode()}")
        if rc != 0:
            raise VspError(f"vsp error {rc}: {self.lib.vsp_last_error(self.h).decode()}")

    def last_error(self):
        return self.lib.vsp_last_error(self.h).decode()

    def set_stream(self, stream_handle):
        self.check(self.lib.vsp_set_stream(self.h, C.c_void_p(stream_handle) if stream_handle else None))

    def synchronize(self):
        self.check(self.lib.vsp_synchronize(self.h))

    def stat(self, name):
        return self.lib.vsp_get_stat(self.h, name.encode())

    def stats_reset(self):
        self.lib.vsp_stats_reset(self.h)

    def set_option(self, name, value):
        self.check(self.lib.vsp_set_option(self.h, name.encode(), int(value)))
        self.options[name] = int(value)

    # ---- raw device memory
    def dmalloc(self, nbytes):
        p = self.lib.vsp_dmalloc(self.h, nbytes)
        if not p:
            raise VspError("vsp_dmalloc failed: " + self.last_error())
        return p

    def dfree(self, p):
        self.lib.vsp_dfree(self.h, C.c_void_p(p))

    def h2d(self, dptr, host):
        host = np.ascontiguousarray(host)
        self.check(self.lib.vsp_h2d(self.h, C.c_void_p(dptr), _ptr(host), host.nbytes))

    def d2h(self, host, dptr):
        self.check(self.lib.vsp_d2h(self.h, _ptr(host), C.c_void_p(dptr), host.nbytes))

    def host_register(self, arr):
        """Page-lock a host array the library copies from on every call (the witness): its transfers become asynchronous DMA."""
        self.check(self.lib.vsp_host_register(self.h, _ptr(arr), arr.nbytes))
        return arr

    def host_unregister(self, arr):
        self.check(self.lib.vsp_host_unregister(self.h, _ptr(arr)))

    def to_device(self, host):
        host = np.ascontiguousarray(host)
        p = self.dmalloc(max(host.nbytes, 16))
        self.h2d(p, host)
        return p

    # ---- bases
    def upload_bases(self, bases, group=1):
        gr = _group(group)
        bases = _u64(bases, gr.affine)
        h = getattr(self.lib, "vsp_bases_upload" + gr.suffix)(self.h, _ptr(bases), bases.shape[0])
        if not h:
            raise VspError("bases upload failed: " + self.last_error())
        return Bases(self, h, group)

    def bases_from_device(self, dptr, n, group=1):
        h = getattr(self.lib, "vsp_bases_from_device" + _group(group).suffix)(self.h, _ptr(dptr), n)
        if not h:
            raise VspError("bases_from_device failed: " + self.last_error())
        return Bases(self, h, group)


class Bases:
    """Device-resident MSM bases (a proving-key query), vsp_bases."""

    def __init__(self, ctx, handle, group):
        self.ctx, self.h, self.group = ctx, handle, group
        self.n = ctx.lib.vsp_bases_count(handle)

    def free(self):
        if self.h and self.ctx.h:
            self.ctx.lib.vsp_bases_free(self.ctx.h, self.h)
        self.h = None

    def precompute(self, window_bits=0, split=False):
        """Store the window multiples 2^(c*w) * P once (16x memory at c = 16); later multi-exponentiations share one bucket set.
        split=True (bases whose scalars are dense, e.g. the H query): the table carries the endomorphism rows for split scalars."""
        fn = self.ctx.lib.vsp_bases_precompute_split if split else self.ctx.lib.vsp_bases_precompute
        self.ctx.check(fn(self.ctx.h, self.h, window_bits))
        return self

    def msm(self, d_scalars, n=None, first=0):
        """sum_i scalars[i] * bases[first+i]; d_scalars is a device pointer / torch tensor.  -> (affine, is_inf)."""
        n = self.n - first if n is None else n
        out = np.zeros(_group(self.group).affine, np.uint64)
        inf = C.c_int(0)
        self.ctx.check(self.ctx.lib.vsp_msm_resident(self.ctx.h, self.h, first, n, _ptr(d_scalars), _ptr(out), C.byref(inf)))
        return out, bool(inf.value)

    def msm_batch(self, d_scalars, batch, n=None, first=0, stride=None):
        """`batch` multi-exponentiations over the same bases in one pass (vsp_msm_resident_batch): vector k at d_scalars + 32 * k * stride
        bytes.  -> (affine [batch, 12 | 24], is_inf [batch])."""
        n = self.n - first if n is None else n
        stride = n if stride is None else stride
        out = np.zeros((batch, _group(self.group).affine), np.uint64)
        inf = np.zeros(batch, np.int32)
        self.ctx.check(self.ctx.lib.vsp_msm_resident_batch(self.ctx.h, self.h, first, n, _ptr(d_scalars), batch, stride, _ptr(out), _ptr(inf)))
        return out, inf.astype(bool)

    def msm_launch(self, slot, d_scalars, n=None, first=0):
        """Enqueue the multi-exponentiation on work slot `slot` (own stream); pair with msm_finish_jacobian(slot)."""
        n = self.n - first if n is None else n
        self.ctx.check(self.ctx.lib.vsp_msm_launch(self.ctx.h, slot, self.h, first, n, _ptr(d_scalars)))

    def msm_finish_jacobian(self, slot):
        out = np.zeros(_group(self.group).jacobian, np.uint64)
        self.ctx.check(self.ctx.lib.vsp_msm_finish_jacobian(self.ctx.h, slot, _ptr(out)))
        return out

    def msm_finish_jacobian_device(self, slot, d_out, stream=None):
        """Same, the record left in DEVICE memory at d_out (pointer / torch tensor) by an asynchronous copy queued on `stream`
        (a hipStream_t handle; None = the context's stream) -- where the RCCL all-gather of the sharded MSM reads it."""
        self.ctx.check(self.ctx.lib.vsp_msm_finish_jacobian_device(self.ctx.h, slot, _ptr(d_out), C.c_void_p(stream) if stream else None))

    def msm_jacobian(self, d_scalars, n=None, first=0):
        """Same, result as the Jacobian partial-sum record (18 / 36 uint64) ranks exchange."""
        n = self.n - first if n is None else n
        out = np.zeros(_group(self.group).jacobian, np.uint64)
        self.ctx.check(self.ctx.lib.vsp_msm_resident_jacobian(self.ctx.h, self.h, first, n, _ptr(d_scalars), _ptr(out)))
        return out


# ---- multiexp (a1-a3) ------------------------------------------------------------------------
def multiexp(ctx, bases, scalars, group=1):
    """algebra::multiexp<multiexp_method_BDLO12>: sum_i scalars[i] * bases[i] as an affine point
    (zero array = infinity).  bases [n,12|24], scalars [n,4], host arrays."""
    gr = _group(group)
    bases, scalars = _u64(bases, gr.affine), _u64(scalars, 4)
    if bases.shape[0] != scalars.shape[0]:
        raise ValueError("multiexp: bases and scalars differ in length")   # the reference asserts equal ranges
    out = np.zeros(gr.affine, np.uint64)
    inf = C.c_int(0)
    ctx.check(getattr(ctx.lib, "vsp_msm" + gr.suffix)(ctx.h, _ptr(bases), _ptr(scalars), bases.shape[0], _ptr(out), C.byref(inf)))
    return out


def multiexp_with_mixed_addition(ctx, bases, scalars, group=1):
    """algebra::multiexp_with_mixed_addition: same value; the 0 / 1 scalar special cases are handled
    inside the bucket pipeline (zero digits are skipped, the ones share one bucket)."""
    return multiexp(ctx, bases, scalars, group)


def fold_jacobian(ctx, records, group=1):
    """Fold Jacobian partial sums (the multi-GPU exchange records) into one affine point."""
    records = _u64(records, _group(group).jacobian)
    out = np.zeros(_group(group).affine, np.uint64)
    inf = C.c_int(0)
    ctx.check(ctx.lib.vsp_fold_jacobian(ctx.h, group, _ptr(records), records.shape[0], _ptr(out), C.byref(inf)))
    return out


def fold_jacobian_device(ctx, d_records, count, group=1, stream=None):
    """Fold `count` records that sit in device memory (the all-gather's output) behind the work already queued on `stream`."""
    out = np.zeros(_group(group).affine, np.uint64)
    inf = C.c_int(0)
    ctx.check(ctx.lib.vsp_fold_jacobian_device(ctx.h, group, _ptr(d_records), count, C.c_void_p(stream) if stream else None, _ptr(out), C.byref(inf)))
    return out


# ---- evaluation_domain (a6) -------------------------------------------------------------------
class EvaluationDomain:
    """math::evaluation_domain<Fr>: the basic radix-2 domain (m a power of two) or the step radix-2 domain (m = big + small,
    both powers of two).  Methods take and return host arrays [m,4] of canonical Fr; *_device variants work in place on device
    memory.  Method names are upstream's (crypto3-math domains/evaluation_domain.hpp); the libfqfft spellings are aliases."""

    def __init__(self, ctx, m, _min_size=None):
        self.ctx, self.h = ctx, None
        if m == 1 and _min_size is None:          # degenerate size kept for completeness: every transform is the identity
            self.m, self.kind = 1, "basic_radix2"
            return
        self.h = ctx.lib.vsp_domain_create(ctx.h, m if _min_size is None else _min_size)
        if not self.h:
            raise ValueError("evaluation_domain: " + ctx.last_error())          # upstream: std::invalid_argument
        self.m = ctx.lib.vsp_domain_size(self.h)
        self.kind = ("basic_radix2", "step_radix2")[ctx.lib.vsp_domain_kind(self.h)]
        if _min_size is None and self.m != m:
            self.free()
            raise ValueError("evaluation_domain: %d is neither a power of two nor big + small with both powers of two" % m)

    def free(self):
        if self.h and self.ctx.h:
            self.ctx.lib.vsp_domain_free(self.ctx.h, self.h)
        self.h = None

    def _vec(self, a, rows=None):
        a = _u64(a, 4).copy()
        if a.shape[0] != (self.m if rows is None else rows):
            raise ValueError("evaluation_domain: expected vector of size m")     # upstream: std::invalid_argument
        return a

    def _run(self, a, inverse, coset):
        a = self._vec(a)
        g = None if coset is None else _u64(coset)
        if self.h is None:
            self.ctx.check(self.ctx.lib.vsp_ntt_fr(self.ctx.h, _ptr(a), 0, int(inverse), _ptr(g)))
        else:
            self.ctx.check(self.ctx.lib.vsp_domain_fft(self.ctx.h, self.h, _ptr(a), int(inverse), _ptr(g)))
        return a

    def fft(self, a): return self._run(a, False, None)
    def inverse_fft(self, a): return self._run(a, True, None)
    def coset_fft(self, a, g): return self._run(a, False, g)
    def inverse_coset_fft(self, a, g): return self._run(a, True, g)
    cosetFFT = coset_fft
    icosetFFT = inverse_coset_fft
    iFFT = inverse_fft
    FFT = fft

    def fft_device(self, d_a, inverse=False, coset=None):
        g = None if coset is None else _u64(coset)
        if self.h is None:
            self.ctx.check(self.ctx.lib.vsp_ntt_fr_device(self.ctx.h, _ptr(d_a), 0, int(inverse), _ptr(g)))
        else:
            self.ctx.check(self.ctx.lib.vsp_domain_fft_device(self.ctx.h, self.h, _ptr(d_a), int(inverse), _ptr(g)))

    def evaluate_all_lagrange_polynomials(self, t):
        out = np.zeros((self.m, 4), np.uint64)
        self.ctx.check(self.ctx.lib.vsp_domain_lagrange(self.ctx.h, self.h, _ptr(_u64(t)), _ptr(out)))
        return out

    def get_domain_element(self, idx):
        out = np.zeros(4, np.uint64)
        self.ctx.check(self.ctx.lib.vsp_domain_element(self.ctx.h, self.h, idx, _ptr(out)))
        return out

    def compute_vanishing_polynomial(self, t):
        out = np.zeros(4, np.uint64)
        self.ctx.check(self.ctx.lib.vsp_domain_vanishing(self.ctx.h, self.h, _ptr(_u64(t)), _ptr(out)))
        return out

    def add_poly_z(self, coeff, H):
        H = self._vec(H, self.m + 1)
        self.ctx.check(self.ctx.lib.vsp_domain_add_poly_z(self.ctx.h, self.h, _ptr(_u64(coeff)), _ptr(H)))
        return H

    def divide_by_z_on_coset(self, P):
        P = self._vec(P)
        self.ctx.check(self.ctx.lib.vsp_domain_divide_by_z_on_coset(self.ctx.h, self.h, _ptr(P)))
        return P

    def witness_map_h(self, Az, Bz, Cz):
        Az, Bz, Cz = (self._vec(x) for x in (Az, Bz, Cz))
        H = np.zeros((self.m, 4), np.uint64)
        self.ctx.check(self.ctx.lib.vsp_domain_witness_map_h(self.ctx.h, self.h, _ptr(Az), _ptr(Bz), _ptr(Cz), _ptr(H)))
        return H


def BasicRadix2Domain(ctx, m):
    if m < 1 or m & (m - 1):
        raise ValueError("basic_radix2_domain: m must be a power of two")       # upstream throws for other sizes
    return EvaluationDomain(ctx, m)


def StepRadix2Domain(ctx, m):
    d = EvaluationDomain(ctx, m)
    if d.kind != "step_radix2":
        d.free()
        raise ValueError("step_radix2_domain: m must be big + small with small < big, both powers of two")
    return d


def make_evaluation_domain(ctx, min_size):
    """math::make_evaluation_domain<Fr>(k): the first of basic_radix2(k), step_radix2(k), basic_radix2(big + rounded_small),
    step_radix2(big + rounded_small) that exists -- the domain r1cs_to_qap works over for k = constraints + inputs + 1."""
    return EvaluationDomain(ctx, None, _min_size=min_size)


def witness_map_h(ctx, Az, Bz, Cz):
    """r1cs_to_qap::witness_map tail (d1=d2=d3=0): coefficients of H from the evaluation vectors over the domain whose size the
    vectors have."""
    m = _u64(Az, 4).shape[0]
    if m == 1:
        Az, Bz, Cz = (_u64(x, 4).copy() for x in (Az, Bz, Cz))
        H = np.zeros((1, 4), np.uint64)
        ctx.check(ctx.lib.vsp_witness_map_h(ctx.h, _ptr(Az), _ptr(Bz), _ptr(Cz), 0, _ptr(H)))
        return H
    d = EvaluationDomain(ctx, m)
    try:
        return d.witness_map_h(Az, Bz, Cz)
    finally:
        d.free()


# ---- Groth16 prover (a8, a9) ---------------------------------------------------------------------
class R1CS:
    """Device-resident constraint system: three CSR matrices (row_ptr u32, col u32, coeff [nnz,4] u64)."""

    def __init__(self, ctx, num_constraints, num_inputs, num_vars, A, B, Cm):
        self.ctx = ctx
        self.num_constraints, self.num_inputs, self.num_vars = num_constraints, num_inputs, num_vars
        args = []
        self._keep = []
        for rp, ci, co in (A, B, Cm):
            rp = np.ascontiguousarray(rp, dtype=np.uint32); ci = np.ascontiguousarray(ci, dtype=np.uint32); co = _u64(co, 4)
            if rp.shape[0] != num_constraints + 1 or ci.shape[0] != rp[-1] or co.shape[0] != rp[-1]:
                raise ValueError("R1CS: malformed CSR")
            self._keep += [rp, ci, co]
            args += [_ptr(rp), _ptr(ci), _ptr(co)]
        self.h = ctx.lib.vsp_r1cs_upload(ctx.h, num_constraints, num_inputs, num_vars, *args)
        if not self.h:
            raise VspError("r1cs upload failed: " + ctx.last_error())
        self._keep = None
        self.m = ctx.lib.vsp_r1cs_domain_size(self.h)              # make_evaluation_domain(num_constraints + num_inputs + 1)
        self.domain_kind = ("basic_radix2", "step_radix2")[ctx.lib.vsp_r1cs_domain_kind(self.h)]

    def check(self, ctx, witnesses):
        """bp.is_satisfied() for many witnesses (vsp_r1cs_check_batch): witnesses [count, num_vars, 4], any count.
        -> (status u8 [count]: 0 satisfied, bit 0 a value >= r, bit 1 some constraint fails; first_bad_row u64 [count]: num_constraints
        when none fails; bad_rows u64 [count])"""
        witnesses = np.ascontiguousarray(witnesses, dtype=np.uint64)
        if witnesses.ndim != 3 or witnesses.shape[1:] != (self.num_vars, 4):
            raise ValueError("R1CS.check: witnesses must be [count, num_vars, 4]")
        n = witnesses.shape[0]
        status = np.zeros(n, np.uint8); first = np.zeros(n, np.uint64); bad = np.zeros(n, np.uint64)
        # sized at least one element, so that count = 0 still passes non-null pointers
        wp = witnesses if witnesses.size else np.zeros(4, np.uint64)
        ctx.check(ctx.lib.vsp_r1cs_check_batch(ctx.h, self.h, _ptr(wp), n, _ptr(status if n else np.zeros(1, np.uint8)), _ptr(first if n else np.zeros(1, np.uint64)),
                                               _ptr(bad if n else np.zeros(1, np.uint64))))
        return status, first, bad

    def check_device(self, ctx, d_witnesses, stride, rows, members=None, count=None):
        """check over witnesses in device memory (vsp_r1cs_check_batch_device): d_witnesses a device pointer to `rows` rows of `stride`
        values of 4 words, members the row of every member (None: rows 0 .. count - 1), any count.  -> as check"""
        mem, n = _device_members(members, count)
        status = np.zeros(max(n, 1), np.uint8); first = np.zeros(max(n, 1), np.uint64); bad = np.zeros(max(n, 1), np.uint64)
        ctx.check(ctx.lib.vsp_r1cs_check_batch_device(ctx.h, self.h, C.c_void_p(int(d_witnesses)), int(stride), int(rows), _ptr(mem) if mem is not None else None, n,
                                                      _ptr(status), _ptr(first), _ptr(bad)))
        return status[:n], first[:n], bad[:n]

    def is_satisfied(self, ctx, witness):
        """bp.is_satisfied() (common.hpp:1109-1128) on the GPU: True exactly when every constraint holds and every value is canonical"""
        witness = _u64(witness, 4)
        if witness.shape[0] != self.num_vars:
            raise ValueError("R1CS.is_satisfied: witness must have num_vars entries (primary || auxiliary)")
        ok = C.c_int(0)
        ctx.check(ctx.lib.vsp_r1cs_is_satisfied(ctx.h, self.h, _ptr(witness if witness.size else np.zeros(4, np.uint64)), C.byref(ok), None))
        return bool(ok.value)

    def free(self):
        if self.h and self.ctx.h:
            self.ctx.lib.vsp_r1cs_free(self.ctx.h, self.h)
        self.h = None


class ProvingKey:
    """r1cs_gg_ppzksnark proving key with device-resident queries."""

    def __init__(self, ctx, alpha_g1, beta_g1, beta_g2, delta_g1, delta_g2, A_query, B_query_g1, B_query_g2, H_query, L_query):
        self.ctx = ctx
        self.queries = (A_query, B_query_g1, B_query_g2, H_query, L_query)
        consts = [_u64(x) for x in (alpha_g1, beta_g1, beta_g2, delta_g1, delta_g2)]
        self.h = ctx.lib.vsp_pk_create(ctx.h, *[_ptr(c) for c in consts], *[q.h for q in self.queries])
        if not self.h:
            raise VspError("pk_create failed: " + ctx.last_error())

    def free(self):
        if self.h and self.ctx.h:
            self.ctx.lib.vsp_pk_free(self.ctx.h, self.h)
        self.h = None


KEY_PARTS = {"A_query": (0, 12), "B_query_g1": (1, 12), "B_query_g2": (2, 24), "H_query": (3, 12), "L_query": (4, 12),
             "gamma_ABC_g1": (5, 12), "alpha_g1": (6, 12), "beta_g1": (7, 12), "delta_g1": (8, 12), "beta_g2": (9, 24),
             "delta_g2": (10, 24), "gamma_g2": (11, 24), "gamma_g1": (12, 12)}


class Keypair:
    """zk::generate<proof_system>(constraint_system) on the GPU with explicit toxic waste [5,4] = (t, alpha, beta, gamma, delta)."""

    def __init__(self, ctx, cs, toxic, precompute=False, precompute_window=0, _handle=None):
        """precompute: False / 0 = a plain key; True / 1 = tables of window multiples on A, B(G1), B(G2), L; else a bit mask (vsp.h; 17 = all
        five queries).  precompute_window: the tables' window in bits (0 = by the query's size).  For batched proving at the real circuit's
        size (2^15..2^16 constraints): precompute=17, precompute_window=14."""
        self.ctx = ctx
        if _handle is None:
            toxic = _u64(toxic).reshape(20)
            if precompute_window:
                ctx.set_option("generate_precompute_window", int(precompute_window))
            try:
                _handle = ctx.lib.vsp_groth16_generate(ctx.h, cs.h, _ptr(toxic), int(precompute))
            finally:
                if precompute_window:
                    ctx.set_option("generate_precompute_window", 0)
            if not _handle:
                raise VspError("groth16_generate failed: " + ctx.last_error())
        self.h = _handle
        self.pk = _BorrowedPk(ctx.lib.vsp_keypair_pk(self.h))

    @classmethod
    def from_blob(cls, ctx, blob, precompute=False):
        """deserialize_pk_crs (common.hpp:749-754): the big-endian "fast" proving-key blob -> a resident key, converted on the GPU."""
        buf = np.frombuffer(bytes(blob), dtype=np.uint8)
        h = ctx.lib.vsp_pk_from_blob(ctx.h, _ptr(buf), buf.shape[0], int(bool(precompute)))
        if not h:
            raise VspError("pk_from_blob failed: " + ctx.last_error())
        return cls(ctx, None, None, _handle=h)

    def to_blob(self):
        out = np.zeros(self.ctx.lib.vsp_pk_blob_size(self.h), np.uint8)
        self.ctx.check(self.ctx.lib.vsp_pk_to_blob(self.ctx.h, self.h, _ptr(out)))
        return out.tobytes()

    def device_bytes(self):
        """device memory the key's six queries hold (points, tables of window multiples, 28-bit-limb copies)"""
        return self.ctx.lib.vsp_keypair_device_bytes(self.h)

    def part(self, name):
        which, width = KEY_PARTS[name]
        n = self.ctx.lib.vsp_keypair_count(self.h, which)
        out = np.zeros((n, width), np.uint64)
        self.ctx.check(self.ctx.lib.vsp_keypair_export(self.ctx.h, self.h, which, _ptr(out)))
        return out

    def free(self):
        if self.h and self.ctx.h:
            self.ctx.lib.vsp_keypair_free(self.ctx.h, self.h)
        self.h = None


class _BorrowedPk:
    def __init__(self, handle):
        self.h = handle


def groth16_prove(ctx, cs, pk, witness, r, s, saver_P1=None, saver_r_enc=None):
    """r1cs_gg_ppzksnark_prover::process with explicit r, s.  -> (A[12], B[24], C[12], proof_bytes[192])."""
    witness = _u64(witness, 4)
    if witness.shape[0] != cs.num_vars:
        raise ValueError("prove: witness must have num_vars entries (primary || auxiliary)")
    A = np.zeros(12, np.uint64); B = np.zeros(24, np.uint64); Cc = np.zeros(12, np.uint64)
    proof = np.zeros(192, np.uint8)
    p1 = None if saver_P1 is None else _u64(saver_P1)
    re = None if saver_r_enc is None else _u64(saver_r_enc)
    _check_single(ctx, ctx.lib.vsp_groth16_prove(ctx.h, cs.h, pk.h, _ptr(witness), _ptr(_u64(r)), _ptr(_u64(s)), _ptr(p1), _ptr(re),
                                                 _ptr(A), _ptr(B), _ptr(Cc), _ptr(proof)))
    return A, B, Cc, proof.tobytes()


def _check_single(ctx, rc):
    """ctx.check for the single-proof calls: an Unsatisfied carries the first failing constraint"""
    try:
        ctx.check(rc)
    except Unsatisfied as e:
        e.first_bad_row = int(ctx.stat("prove_first_bad_row"))
        raise


def _check_batch(ctx, rc, results):
    """ctx.check for the batch calls: an Unsatisfied carries the members' verdicts and the batch's outputs"""
    try:
        ctx.check(rc)
    except Unsatisfied as e:
        e.status, e.first_bad_row = groth16_prove_batch_verdicts(ctx, len(results[3]))
        e.results = results
        raise
    return results


def groth16_prove_batch_verdicts(ctx, count=None):
    """the verdicts of the last batch that finished on this context with option prove_check_witness = 1
    -> (status u8 [K]: 0 or bit 1 = unsatisfied, first_bad_row u64 [K]); count: K when the batch was not proved through this module"""
    K = count if count is not None else getattr(ctx, "_prove_batch_last", 0)
    status = np.zeros(max(K, 1), np.uint8); first = np.zeros(max(K, 1), np.uint64)
    ctx.check(ctx.lib.vsp_groth16_prove_batch_verdicts(ctx.h, _ptr(status), _ptr(first)))
    return status[:K], first[:K]


def _batch_inputs(cs, witnesses, r, s):
    """witnesses [K, num_vars, 4], r / s [K, 4] as contiguous uint64 arrays -> (witnesses, r, s, K)"""
    witnesses = np.ascontiguousarray(witnesses, dtype=np.uint64)
    if witnesses.ndim != 3 or witnesses.shape[1:] != (cs.num_vars, 4):
        raise ValueError("prove_batch: witnesses must be [K, num_vars, 4]")
    K = witnesses.shape[0]
    r = np.ascontiguousarray(r, dtype=np.uint64).reshape(K, 4); s = np.ascontiguousarray(s, dtype=np.uint64).reshape(K, 4)
    return witnesses, r, s, K


def groth16_prove_batch(ctx, cs, pk, witnesses, r, s):
    """K proofs over one key in one pass (vsp_groth16_prove_batch): witnesses [K, num_vars, 4], r / s [K, 4].  The key is plain, or has
    tables of window multiples of at most 16 bits (refused otherwise, and with option msm_batch_tables = 0).
    -> (A [K, 12], B [K, 24], C [K, 12], [proof bytes] * K); proof k is byte-identical to groth16_prove(witness_k, r_k, s_k)."""
    witnesses, r, s, K = _batch_inputs(cs, witnesses, r, s)
    A = np.zeros((K, 12), np.uint64); B = np.zeros((K, 24), np.uint64); Cc = np.zeros((K, 12), np.uint64)
    proofs = np.zeros((K, 192), np.uint8)
    ctx._prove_batch_last = K
    rc = ctx.lib.vsp_groth16_prove_batch(ctx.h, cs.h, pk.h, _ptr(witnesses), K, _ptr(r), _ptr(s), _ptr(A), _ptr(B), _ptr(Cc), _ptr(proofs))
    return _check_batch(ctx, rc, (A, B, Cc, [proofs[k].tobytes() for k in range(K)]))


def _device_members(members, count):
    """the `members` map of the calls over witnesses in device memory: (u32 array or None, count)"""
    if members is None:
        if count is None:
            raise ValueError("witnesses in device memory: members or count is needed")
        return None, int(count)
    mem = np.ascontiguousarray(members, dtype=np.uint32).reshape(-1)
    return mem, mem.shape[0]


def groth16_prove_batch_launch_device(ctx, cs, pk, d_witnesses, stride, rows, r, s, members=None, count=None):
    """groth16_prove_batch_launch over witnesses in device memory (vsp_groth16_prove_batch_launch_device): d_witnesses a device pointer
    to `rows` rows of `stride` >= num_vars values of 4 canonical words, complete on the context's stream; member k is row members[k]
    (None: rows 0 .. count - 1).  Nothing is waited for; every read of the buffer is queued on the context's stream when this
    returns.  Finish with groth16_prove_batch_finish.  Returns K."""
    mem, K = _device_members(members, count)
    r = np.ascontiguousarray(r, dtype=np.uint64).reshape(-1, 4); s = np.ascontiguousarray(s, dtype=np.uint64).reshape(-1, 4)
    if r.shape[0] != K or s.shape[0] != K:
        raise ValueError("prove_batch_device: r and s must be [K, 4]")
    ctx.check(ctx.lib.vsp_groth16_prove_batch_launch_device(ctx.h, cs.h, pk.h, C.c_void_p(int(d_witnesses)), int(stride), int(rows), _ptr(mem) if mem is not None else None,
                                                            K, _ptr(r), _ptr(s)))
    ctx._prove_batch_count = K
    return K


def groth16_prove_batch_device(ctx, cs, pk, d_witnesses, stride, rows, r, s, members=None, count=None):
    """K proofs from witnesses in device memory: launch_device + finish.  -> as groth16_prove_batch, byte for byte"""
    groth16_prove_batch_launch_device(ctx, cs, pk, d_witnesses, stride, rows, r, s, members, count)
    return groth16_prove_batch_finish(ctx)


def groth16_prove_batch_launch(ctx, cs, pk, witnesses, r, s):
    """first half of groth16_prove_batch: copy the witnesses, queue every kernel of the K proofs, return K (one batch in flight per context)"""
    witnesses, r, s, K = _batch_inputs(cs, witnesses, r, s)
    ctx.check(ctx.lib.vsp_groth16_prove_batch_launch(ctx.h, cs.h, pk.h, _ptr(witnesses), K, _ptr(r), _ptr(s)))
    ctx._prove_batch_count = K
    return K


def groth16_prove_batch_finish(ctx):
    """second half: -> (A [K, 12], B [K, 24], C [K, 12], [proof bytes] * K) of the batch of K launched on this context"""
    K = getattr(ctx, "_prove_batch_count", 0)
    if not K:
        raise RuntimeError("prove_batch_finish: no batch in flight on this context")
    ctx._prove_batch_count = 0
    A = np.zeros((K, 12), np.uint64); B = np.zeros((K, 24), np.uint64); Cc = np.zeros((K, 12), np.uint64)
    proofs = np.zeros((K, 192), np.uint8)
    ctx._prove_batch_last = K
    rc = ctx.lib.vsp_groth16_prove_batch_finish(ctx.h, _ptr(A), _ptr(B), _ptr(Cc), _ptr(proofs))
    return _check_batch(ctx, rc, (A, B, Cc, [proofs[k].tobytes() for k in range(K)]))


class PackedWitness:
    """the witness in the packed form of vsp_witness_pack: two class bits per wire, per-word offsets, the dense values"""

    def __init__(self, witness):
        witness = _u64(witness, 4)
        lib = _lib.load()
        self.num_vars = witness.shape[0]
        words = lib.vsp_witness_pack_words(self.num_vars)
        self.class_words = np.zeros(words, np.uint64); self.word_offsets = np.zeros(words, np.uint32)
        n = C.c_size_t(0)
        if lib.vsp_witness_pack(_ptr(witness), self.num_vars, _ptr(self.class_words), _ptr(self.word_offsets), None, 0, C.byref(n)) != 0:
            raise ValueError("witness_pack failed")
        self.dense = np.zeros((max(n.value, 1), 4), np.uint64)
        if lib.vsp_witness_pack(_ptr(witness), self.num_vars, _ptr(self.class_words), _ptr(self.word_offsets), _ptr(self.dense), n.value, C.byref(n)) != 0:
            raise ValueError("witness_pack failed")
        self.n_dense = n.value

    @property
    def nbytes(self):
        return self.class_words.nbytes + self.word_offsets.nbytes + self.n_dense * 32


def groth16_prove_launch(ctx, cs, pk, witness, r, s, saver_P1=None, saver_r_enc=None):
    """first half of groth16_prove: queue the whole proof on the context's streams and return (one proof in flight per context).
    witness: an array [num_vars, 4] (keep it alive and unchanged until the finish when it is page-locked) or a PackedWitness."""
    p1 = None if saver_P1 is None else _u64(saver_P1)
    re = None if saver_r_enc is None else _u64(saver_r_enc)
    r, s = _u64(r), _u64(s)
    if isinstance(witness, PackedWitness):
        if witness.num_vars != cs.num_vars:
            raise ValueError("prove: witness must have num_vars entries (primary || auxiliary)")
        ctx.check(ctx.lib.vsp_groth16_prove_launch_packed(ctx.h, cs.h, pk.h, _ptr(witness.class_words), _ptr(witness.word_offsets), _ptr(witness.dense),
                                                          witness.n_dense, _ptr(r), _ptr(s), _ptr(p1), _ptr(re)))
        return
    witness = _u64(witness, 4)
    if witness.shape[0] != cs.num_vars:
        raise ValueError("prove: witness must have num_vars entries (primary || auxiliary)")
    ctx.check(ctx.lib.vsp_groth16_prove_launch(ctx.h, cs.h, pk.h, _ptr(witness), _ptr(r), _ptr(s), _ptr(p1), _ptr(re)))


def groth16_prove_finish(ctx):
    """second half: host-side assembly work, the wait, the proof.  -> (A[12], B[24], C[12], proof_bytes[192])"""
    A = np.zeros(12, np.uint64); B = np.zeros(24, np.uint64); Cc = np.zeros(12, np.uint64)
    proof = np.zeros(192, np.uint8)
    _check_single(ctx, ctx.lib.vsp_groth16_prove_finish(ctx.h, _ptr(A), _ptr(B), _ptr(Cc), _ptr(proof)))
    return A, B, Cc, proof.tobytes()


# ---- SAVER wrapper (f.3): elgamal_verifiable over BLS12-381 around the prover ---------------------------------------------
def saver_generate_keypair(ctx, rnd, gamma_abc_g1, delta_g1, gamma_g1, msg_size):
    """generate_keypair<elgamal_verifiable>(rnd, {gg_keypair, msg_size}) (common.hpp:921-931) with the 3 * msg_size + 2 random scalars
    explicit.  -> (public key words, secret key rho [4], verification key words)"""
    n = int(msg_size)
    rnd = _u64(rnd, 4)
    if rnd.shape[0] != 3 * n + 2:
        raise ValueError("generate_keypair: 3 * msg_size + 2 random values are needed")
    gabc = _u64(gamma_abc_g1, 12)
    if gabc.shape[0] < n + 1:
        raise ValueError("generate_keypair: the verification key has fewer than msg_size + 1 accumulation elements")
    pk = np.zeros(ctx.lib.vsp_saver_pk_words(n), np.uint64); sk = np.zeros(4, np.uint64); vk = np.zeros(ctx.lib.vsp_saver_vk_words(n), np.uint64)
    ctx.check(ctx.lib.vsp_saver_keygen(ctx.h, n, _ptr(_u64(delta_g1)), _ptr(_u64(gamma_g1)), _ptr(gabc), _ptr(rnd), _ptr(pk), _ptr(sk), _ptr(vk)))
    return pk, sk, vk


class SaverPublicKey:
    """elgamal_verifiable public key resident for many votes (fixed-base tables of its bases)."""

    def __init__(self, ctx, pk_words, gamma_abc_g1, msg_size):
        self.ctx, self.n = ctx, int(msg_size)
        self.words = _u64(pk_words).reshape(-1)
        gabc = _u64(gamma_abc_g1, 12)
        # the C side reads vsp_saver_pk_words(n) words and n + 1 accumulation elements unconditionally (the C ABI carries no lengths)
        if self.n < 1 or self.words.shape[0] != ctx.lib.vsp_saver_pk_words(self.n):
            raise ValueError("SaverPublicKey: the flat public key must have vsp_saver_pk_words(msg_size) words")
        if gabc.shape[0] < self.n + 1:
            raise ValueError("SaverPublicKey: the verification key has fewer than msg_size + 1 accumulation elements")
        self.h = ctx.lib.vsp_saver_pk_load(ctx.h, self.n, _ptr(self.words), _ptr(gabc))
        if not self.h:
            raise VspError("saver_pk_load failed: " + ctx.last_error())

    def upload(self, ctx=None):
        """build the tables of all 3 msg_size + 3 fixed points and put them on the context's device (vsp_saver_pk_upload); the batch
        calls do it themselves, and a second call does nothing"""
        ctx = ctx or self.ctx
        ctx.check(ctx.lib.vsp_saver_pk_upload(ctx.h, self.h))

    @property
    def device_bytes(self):
        return int(self.ctx.lib.vsp_saver_pk_device_bytes(self.h))

    def free(self):
        if self.h and self.ctx.h:
            self.ctx.lib.vsp_saver_pk_free(self.ctx.h, self.h)
        self.h = None


def saver_encrypt(ctx, spk, cs, pk, msg, witness, r_enc, r, s):
    """encrypt<elgamal_verifiable, verifiable_encryption>(m, {r_enc, pk_eid, gg_keypair, primary, auxiliary}) (common.hpp:1131-1135):
    -> (ciphertext [msg_size + 2, 12], (A, B, C), proof bytes)"""
    witness = _u64(witness, 4); msg = _u64(msg, 4)
    if witness.shape[0] != cs.num_vars or msg.shape[0] != spk.n:
        raise ValueError("encrypt: witness must have num_vars entries and the message msg_size blocks")
    ct = np.zeros((spk.n + 2, 12), np.uint64)
    A = np.zeros(12, np.uint64); B = np.zeros(24, np.uint64); Cc = np.zeros(12, np.uint64); proof = np.zeros(192, np.uint8)
    _check_single(ctx, ctx.lib.vsp_saver_encrypt(ctx.h, spk.h, cs.h, pk.h, _ptr(msg), _ptr(witness), _ptr(_u64(r_enc)), _ptr(_u64(r)), _ptr(_u64(s)),
                                                 _ptr(ct), _ptr(A), _ptr(B), _ptr(Cc), _ptr(proof)))
    return ct, (A, B, Cc), proof.tobytes()


def saver_ciphertext_batch(ctx, spk, msgs, r_enc, addends=True, blobs=True):
    """the ciphertexts of K ballots on the GPU (vsp_saver_ciphertext_batch): msgs [K, msg_size, 4], r_enc [K, 4]
    -> (ct [K, msg_size + 2, 12], addends [K, 12] = r_enc_k gamma_inverse_sum_s_g1 or None, [blob bytes] * K or None)"""
    msgs = np.ascontiguousarray(msgs, dtype=np.uint64).reshape(-1, spk.n, 4)
    K = msgs.shape[0]
    r_enc = np.ascontiguousarray(r_enc, dtype=np.uint64).reshape(K, 4)
    ct = np.zeros((K, spk.n + 2, 12), np.uint64)
    add = np.zeros((K, 12), np.uint64) if addends else None
    bl = np.zeros((K, ctx.lib.vsp_g1_vector_blob_size(spk.n + 2)), np.uint8) if blobs else None
    ctx.check(ctx.lib.vsp_saver_ciphertext_batch(ctx.h, spk.h, _ptr(msgs), _ptr(r_enc), K, _ptr(ct), _ptr(add), _ptr(bl)))
    return ct, add, None if bl is None else [bl[k].tobytes() for k in range(K)]


def saver_encrypt_batch_launch(ctx, spk, cs, pk, msgs, witnesses, r_enc, r, s):
    """first half of saver_encrypt_batch: every member checked, the K proofs and the ciphertext kernels queued; returns K"""
    witnesses, r, s, K = _batch_inputs(cs, witnesses, r, s)
    msgs = np.ascontiguousarray(msgs, dtype=np.uint64)
    if msgs.shape != (K, spk.n, 4):
        raise ValueError("encrypt_batch: msgs must be [K, msg_size, 4]")
    r_enc = np.ascontiguousarray(r_enc, dtype=np.uint64).reshape(K, 4)
    ctx.check(ctx.lib.vsp_saver_encrypt_batch_launch(ctx.h, spk.h, cs.h, pk.h, _ptr(msgs), _ptr(witnesses), K, _ptr(r_enc), _ptr(r), _ptr(s)))
    ctx._saver_batch = (K, spk.n)
    return K


def saver_encrypt_batch_launch_device(ctx, spk, cs, pk, d_witnesses, stride, rows, r_enc, r, s, members=None, count=None):
    """saver_encrypt_batch_launch over witnesses in device memory (vsp_saver_encrypt_batch_launch_device; the source as in
    groth16_prove_batch_launch_device).  No msgs: the message is the first msg_size values of each member's row.  Returns K."""
    mem, K = _device_members(members, count)
    rnd = [np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 4) for x in (r_enc, r, s)]
    if any(x.shape[0] != K for x in rnd):
        raise ValueError("encrypt_batch_device: r_enc, r and s must be [K, 4]")
    ctx.check(ctx.lib.vsp_saver_encrypt_batch_launch_device(ctx.h, spk.h, cs.h, pk.h, C.c_void_p(int(d_witnesses)), int(stride), int(rows),
                                                            _ptr(mem) if mem is not None else None, K, _ptr(rnd[0]), _ptr(rnd[1]), _ptr(rnd[2])))
    ctx._saver_batch = (K, spk.n)
    return K


def saver_encrypt_batch_device(ctx, spk, cs, pk, d_witnesses, stride, rows, r_enc, r, s, members=None, count=None):
    """K ballots from witnesses in device memory: launch_device + finish.  -> as saver_encrypt_batch, byte for byte"""
    saver_encrypt_batch_launch_device(ctx, spk, cs, pk, d_witnesses, stride, rows, r_enc, r, s, members, count)
    return saver_encrypt_batch_finish(ctx)


def saver_encrypt_batch_finish(ctx):
    """second half: -> (ct [K, msg_size + 2, 12], (A [K, 12], B [K, 24], C [K, 12]), [proof bytes] * K, [ciphertext blob bytes] * K).
    With option prove_check_witness an Unsatisfied carries .status, .first_bad_row and .results = these outputs (zero for its members)."""
    K, n = getattr(ctx, "_saver_batch", None) or (0, 0)
    ctx._saver_batch = None
    if not K:
        ctx.check(ctx.lib.vsp_saver_encrypt_batch_finish(ctx.h, None, None, None, None, None, None))      # the library's refusal
    ct = np.zeros((K, n + 2, 12), np.uint64)
    A = np.zeros((K, 12), np.uint64); B = np.zeros((K, 24), np.uint64); Cc = np.zeros((K, 12), np.uint64)
    proofs = np.zeros((K, 192), np.uint8); bl = np.zeros((K, ctx.lib.vsp_g1_vector_blob_size(n + 2)), np.uint8)
    ctx._prove_batch_last = K
    rc = ctx.lib.vsp_saver_encrypt_batch_finish(ctx.h, _ptr(ct), _ptr(A), _ptr(B), _ptr(Cc), _ptr(proofs), _ptr(bl))
    results = (ct, (A, B, Cc), [proofs[k].tobytes() for k in range(K)], [bl[k].tobytes() for k in range(K)])
    try:
        ctx.check(rc)
    except Unsatisfied as e:
        e.status, e.first_bad_row = groth16_prove_batch_verdicts(ctx, K)
        e.results = results
        raise
    return results


def saver_encrypt_batch(ctx, spk, cs, pk, msgs, witnesses, r_enc, r, s):
    """K ballots of one election in one pass (vsp_saver_encrypt_batch): member k is byte-identical to saver_encrypt(msgs[k], witnesses[k],
    r_enc[k], r[k], s[k]).  -> as saver_encrypt_batch_finish"""
    saver_encrypt_batch_launch(ctx, spk, cs, pk, msgs, witnesses, r_enc, r, s)
    return saver_encrypt_batch_finish(ctx)


def saver_rerandomize(ctx, spk, delta_g2, rnd3, ct, proof_abc):
    """rerandomize<elgamal_verifiable>(rnd[3], ct, {pk_eid, gg_keypair, proof}) (common.hpp:1138-1145), rnd3 = (r', z1, z2)."""
    ct = _u64(ct, 12).copy()
    A, B, Cc = (_u64(x).copy() for x in proof_abc)
    if ct.shape[0] != spk.n + 2 or A.size != 12 or B.size != 24 or Cc.size != 12 or _u64(delta_g2).size != 24 or _u64(rnd3).size != 12:
        raise ValueError("rerandomize: ciphertext of msg_size + 2 points, proof (A[12], B[24], C[12]), delta_g2[24] and three random scalars expected")
    proof = np.zeros(192, np.uint8)
    ctx.check(ctx.lib.vsp_saver_rerandomize(ctx.h, spk.h, _ptr(_u64(delta_g2)), _ptr(_u64(rnd3).reshape(12)), _ptr(ct), _ptr(A), _ptr(B), _ptr(Cc), _ptr(proof)))
    return ct, (A, B, Cc), proof.tobytes()


class SaverRerandomizer:
    """the public data of one election that rerandomizes its ballots in batches (vsp_saver_rerandomizer): the key with its device tables
    and the table of delta_g2.  The key must outlive it."""

    def __init__(self, ctx, spk, delta_g2):
        self.ctx, self.spk, self.n = ctx, spk, spk.n
        d2 = _u64(delta_g2).reshape(-1)
        if d2.size != 24:
            raise ValueError("SaverRerandomizer: delta_g2 is one G2 point of 24 words")
        self.h = ctx.lib.vsp_saver_rerandomizer_new(ctx.h, spk.h, _ptr(d2))
        if not self.h:
            raise VspError("saver_rerandomizer_new failed: " + ctx.last_error())

    @property
    def device_bytes(self):
        return int(self.ctx.lib.vsp_saver_rerandomizer_device_bytes(self.h))

    def free(self):
        if self.h and self.ctx.h:
            self.ctx.lib.vsp_saver_rerandomizer_free(self.ctx.h, self.h)
        self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def saver_rerandomize_batch(ctx, rr, rnd, ct, proofs_abc, proofs=True, blobs=True, status=True, in_place=False):
    """K ballots rerandomized on the GPU (vsp_saver_rerandomize_batch): rnd [K, 3, 4] = (r', z1, z2) of every member, ct [K, msg_size + 2, 12],
    proofs_abc = (A [K, 12], B [K, 24], C [K, 12]); member k is byte-identical to saver_rerandomize on the same inputs.
    -> (ct', (A', B', C'), [proof bytes] * K or None, [ciphertext blob bytes] * K or None, status [K] or None).  A member with a point
    that is no curve point has status 1 and all-zero outputs; with status=False such a member raises instead.  in_place: the outputs
    are written over ct and proofs_abc, which must then be contiguous uint64 arrays."""
    n = rr.n
    ct = np.ascontiguousarray(ct, dtype=np.uint64).reshape(-1, n + 2, 12)
    K = ct.shape[0]
    rnd = np.ascontiguousarray(rnd, dtype=np.uint64).reshape(K, 12)
    A, B, Cc = (np.ascontiguousarray(x, dtype=np.uint64).reshape(K, w) for x, w in zip(proofs_abc, (12, 24, 12)))
    if in_place:
        ct2, A2, B2, C2 = ct, A, B, Cc
    else:
        ct2, A2, B2, C2 = np.zeros_like(ct), np.zeros_like(A), np.zeros_like(B), np.zeros_like(Cc)
    pr = np.zeros((K, 192), np.uint8) if proofs else None
    bl = np.zeros((K, ctx.lib.vsp_g1_vector_blob_size(n + 2)), np.uint8) if blobs else None
    st = np.zeros(K, np.uint8) if status else None
    ctx.check(ctx.lib.vsp_saver_rerandomize_batch(ctx.h, rr.h, _ptr(rnd), _ptr(ct), _ptr(A), _ptr(B), _ptr(Cc), K, _ptr(ct2), _ptr(A2), _ptr(B2), _ptr(C2),
                                                  _ptr(pr), _ptr(bl), _ptr(st)))
    return (ct2, (A2, B2, C2), None if pr is None else [pr[k].tobytes() for k in range(K)], None if bl is None else [bl[k].tobytes() for k in range(K)], st)


def fixed_base_mul(ctx, d_scalars, n, group=1):
    """Generator-side batch_exp: device array out[i] = scalars[i] * generator (canonical affine).  Returns a device pointer."""
    gr = _group(group)
    d_out = ctx.dmalloc(max(n, 1) * 8 * gr.affine)
    ctx.check(getattr(ctx.lib, "vsp_fixed_base_mul" + gr.suffix)(ctx.h, _ptr(d_scalars), n, C.c_void_p(d_out)))
    return d_out


def g1_compress(affine):
    out = np.zeros(48, np.uint8)
    if _lib.load().vsp_g1_compress(_ptr(_u64(affine).reshape(12)), _ptr(out)) != 0:
        raise ValueError("g1_compress: a coordinate is not canonical (>= p)")
    return out.tobytes()


def g2_compress(affine):
    out = np.zeros(96, np.uint8)
    if _lib.load().vsp_g2_compress(_ptr(_u64(affine).reshape(24)), _ptr(out)) != 0:
        raise ValueError("g2_compress: a coordinate is not canonical (>= p)")
    return out.tobytes()


def g1_decompress(data, check_subgroup=True):
    """48 ZCash-compressed bytes -> affine limbs [12] (all zero for infinity); ValueError for an invalid encoding."""
    buf = (C.c_uint8 * 48).from_buffer_copy(bytes(data))
    out = np.zeros(12, np.uint64); inf = C.c_int(0)
    if _lib.load().vsp_g1_decompress(buf, int(check_subgroup), _ptr(out), C.byref(inf)) != 0:
        raise ValueError("g1_decompress: invalid encoding")
    return out


def g2_decompress(data, check_subgroup=True):
    """96 ZCash-compressed bytes -> affine limbs [24] (all zero for infinity); ValueError for an invalid encoding."""
    buf = (C.c_uint8 * 96).from_buffer_copy(bytes(data))
    out = np.zeros(24, np.uint64); inf = C.c_int(0)
    if _lib.load().vsp_g2_decompress(buf, int(check_subgroup), _ptr(out), C.byref(inf)) != 0:
        raise ValueError("g2_decompress: invalid encoding")
    return out


def _decompress_batch(ctx, data, group, check_subgroup):
    """the body of g1_decompress_batch / g2_decompress_batch: records of 48 * group bytes, points of 12 * group limbs"""
    name, size = "g%d_decompress_batch" % group, 48 * group
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    if buf.shape[0] % size:
        raise ValueError("%s: the input is not a whole number of %d-byte points" % (name, size))
    n = buf.shape[0] // size
    out = np.zeros((n, 12 * group), np.uint64); status = np.zeros(n, np.uint8)
    ctx.check(getattr(ctx.lib, "vsp_" + name)(ctx.h, _ptr(buf), n, int(check_subgroup), _ptr(out), _ptr(status)))
    return out, status


def g1_decompress_batch(ctx, data, check_subgroup=True):
    """n x 48 ZCash-compressed bytes -> (points [n,12], status [n]) on the GPU.  status 0 = accepted; bit 0 malformed encoding, bit 1
    no curve point has this x, bit 2 outside the order-r subgroup (only with check_subgroup).  Rejected points and infinity are all zero."""
    return _decompress_batch(ctx, data, 1, check_subgroup)


def g2_decompress_batch(ctx, data, check_subgroup=True):
    """n x 96 ZCash-compressed bytes -> (points [n,24], status [n]) on the GPU.  status 0 = accepted; bit 0 malformed encoding, bit 1
    no point of the twist has this x, bit 2 outside the order-r subgroup (only with check_subgroup).  Rejected points and infinity are
    all zero."""
    return _decompress_batch(ctx, data, 2, check_subgroup)


def proofs_from_blob_batch(ctx, data, check_subgroup=True):
    """n x 192 bytes of proof blobs (A | B | C, back to back) -> (A [n,12], B [n,24], C [n,12], status [n]) on the GPU.  status 0 =
    accepted; bits 0..2 are the OR of the three points' status bits (as g1_decompress_batch), bits 4, 5, 6 say that A, B, C was
    rejected.  Every member of a rejected proof is all zero."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    if buf.shape[0] % 192:
        raise ValueError("proofs_from_blob_batch: the input is not a whole number of 192-byte proofs")
    n = buf.shape[0] // 192
    A = np.zeros((n, 12), np.uint64); B = np.zeros((n, 24), np.uint64); Cc = np.zeros((n, 12), np.uint64); status = np.zeros(n, np.uint8)
    ctx.check(ctx.lib.vsp_proof_from_blob_batch(ctx.h, _ptr(buf), n, int(check_subgroup), _ptr(A), _ptr(B), _ptr(Cc), _ptr(status)))
    return A, B, Cc, status


class Tally:
    """The aggregation of the tally (common.hpp:1193-1216, repeated by every verifier at :1257-1279): ct_len = msg_size + 2 running sums
    of ciphertext components over the ballots added so far (vsp_tally)."""

    def __init__(self, ctx, ct_len):
        self.ctx = ctx
        self.ct_len = int(ct_len)
        self.h = ctx.lib.vsp_tally_create(ctx.h, self.ct_len)
        if not self.h:
            raise VspError("vsp_tally_create failed: " + ctx.last_error())

    def free(self):
        if self.h:
            self.ctx.lib.vsp_tally_free(self.ctx.h, self.h)
            self.h = None

    def add_blobs(self, blobs, check_subgroup=True):
        """blobs: the ballots' G1 vector blobs back to back as one bytes object, or a list of per-ballot blobs (8 + 48 ct_len bytes each).
        Adds every accepted ballot; returns (status [count] uint8, accepted)."""
        data = bytes(blobs) if isinstance(blobs, (bytes, bytearray, memoryview)) else b"".join(bytes(b) for b in blobs)
        size = 8 + 48 * self.ct_len
        if len(data) % size:
            raise ValueError(f"Tally.add_blobs: the input is not a whole number of {size}-byte ballots")
        count = len(data) // size
        status = np.zeros(count, np.uint8); accepted = C.c_size_t(0)
        if count:
            buf = np.frombuffer(data, dtype=np.uint8)
            self.ctx.check(self.ctx.lib.vsp_tally_add_blobs(self.ctx.h, self.h, _ptr(buf), count, int(check_subgroup), _ptr(status), C.byref(accepted)))
        return status, accepted.value

    def result(self):
        """(ct [ct_len,12] canonical affine sums, infinity all zero; ballots accepted since creation or the last reset)"""
        ct = np.zeros((self.ct_len, 12), np.uint64); ballots = C.c_uint64(0)
        self.ctx.check(self.ctx.lib.vsp_tally_result(self.ctx.h, self.h, _ptr(ct), C.byref(ballots)))
        return ct, ballots.value

    def reset(self):
        self.ctx.check(self.ctx.lib.vsp_tally_reset(self.ctx.h, self.h))


def multi_pairing_batch(ctx, g1, g2, m=1, want_gt=True):
    """n products of m pairings each on the GPU: g1 [n*m,12], g2 [n*m,24] canonical affine limbs (all zero = infinity), product i over
    pairs i*m .. i*m + m - 1.  Returns (gt [n,576] uint8 or None, is_one [n] uint8).  The pairing is the test oracle's (pairing.py: no
    conjugation for the negative curve parameter); points are assumed to be in the order-r subgroups.  VspError for a coordinate >= p
    or a point off its curve."""
    g1 = _u64(g1, 12); g2 = _u64(g2, 24); m = int(m)
    if m < 1 or g1.shape[0] != g2.shape[0] or g1.shape[0] % m:
        raise ValueError("multi_pairing_batch: as many G1 as G2 points, a whole number of products of m >= 1 pairs")
    n = g1.shape[0] // m
    gt = np.zeros((n, 576), np.uint8) if want_gt else None
    is_one = np.zeros(n, np.uint8)
    ctx.check(ctx.lib.vsp_multi_pairing_batch(ctx.h, _ptr(g1), _ptr(g2), m, n, _ptr(gt), _ptr(is_one)))
    return gt, is_one


def pairing_batch(ctx, g1, g2):
    """e(g1[i], g2[i]) for every i: [n,576] uint8"""
    return multi_pairing_batch(ctx, g1, g2, 1)[0]


class VerifyingKey:
    """A Groth16 verification key resident on the GPU (vsp_vk): e(alpha_g1, beta_g2), -gamma_g2, -delta_g2 and the multiples of the
    gamma_ABC points."""

    def __init__(self, ctx, alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1):
        self.ctx = ctx
        gabc = _u64(gamma_abc_g1, 12)
        self.n_abc = gabc.shape[0]
        a = _u64(alpha_g1).reshape(12); b = _u64(beta_g2).reshape(24); g = _u64(gamma_g2).reshape(24); d = _u64(delta_g2).reshape(24)
        self.h = ctx.lib.vsp_vk_create(ctx.h, _ptr(a), _ptr(b), _ptr(g), _ptr(d), _ptr(gabc), self.n_abc)
        if not self.h:
            raise VspError("vsp_vk_create failed: " + ctx.last_error())

    def free(self):
        if self.h:
            self.ctx.lib.vsp_vk_free(self.ctx.h, self.h)
            self.h = None

    def alpha_beta(self):
        """e(alpha_g1, beta_g2) as the 576 bytes vk_to_blob takes"""
        gt = np.zeros(576, np.uint8)
        self.ctx.check(self.ctx.lib.vsp_vk_alpha_beta(self.h, _ptr(gt)))
        return gt.tobytes()


def groth16_verify_batch(ctx, vk, inputs, A, B, Cc):
    """Exact verdicts of n proofs: inputs [n, n_abc - 1, 4] canonical scalars, A [n,12], B [n,24], C [n,12] -> [n] uint8, 1 = accepted.
    A proof with a coordinate >= p, a point off its curve or a scalar >= r is rejected; the points are assumed to be in the subgroups
    (decode with check_subgroup)."""
    A = _u64(A, 12); B = _u64(B, 24); Cc = _u64(Cc, 12)
    n = A.shape[0]
    inputs = _u64(inputs).reshape(n, -1) if vk.n_abc > 1 else np.zeros((n, 4), np.uint64)
    if B.shape[0] != n or Cc.shape[0] != n or (vk.n_abc > 1 and inputs.shape[1] != 4 * (vk.n_abc - 1)):
        raise ValueError("groth16_verify_batch: n proofs (A[12], B[24], C[12]) and n x (n_abc - 1) public inputs expected")
    verdict = np.zeros(n, np.uint8)
    ctx.check(ctx.lib.vsp_groth16_verify_batch(ctx.h, vk.h, _ptr(inputs), _ptr(A), _ptr(B), _ptr(Cc), n, _ptr(verdict)))
    return verdict


class SaverVerifier:
    """The verifying side of a SAVER election resident on the GPU (vsp_saver_verifier): the Groth16 verification key as VerifyingKey
    holds it, and the prepared Miller-loop lines of the fixed G2 arguments t_g2[0..msg_size], -H, -gamma_g2, -delta_g2 (and beta_g2, for
    saver_verify_batch_screened).  pk_words is
    the flat public key of saver_generate_keypair."""

    def __init__(self, ctx, pk_words, alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1, msg_size):
        self.ctx = ctx
        self.msg_size = int(msg_size)
        gabc = _u64(gamma_abc_g1, 12)
        self.n_abc = gabc.shape[0]
        words = _u64(pk_words).reshape(-1)
        if self.msg_size < 1 or words.shape[0] != ctx.lib.vsp_saver_pk_words(self.msg_size):
            raise ValueError("SaverVerifier: pk_words is not a public key of this msg_size")
        a = _u64(alpha_g1).reshape(12); b = _u64(beta_g2).reshape(24); g = _u64(gamma_g2).reshape(24); d = _u64(delta_g2).reshape(24)
        self.h = ctx.lib.vsp_saver_verifier_create(ctx.h, self.msg_size, _ptr(words), _ptr(a), _ptr(b), _ptr(g), _ptr(d), _ptr(gabc), self.n_abc)
        if not self.h:
            raise VspError("vsp_saver_verifier_create failed: " + ctx.last_error())

    def free(self):
        if self.h:
            self.ctx.lib.vsp_saver_verifier_free(self.ctx.h, self.h)
            self.h = None


def saver_verify_batch(ctx, ver, ct, inputs_rest, A, B, Cc):
    """verify_encryption of n ballots: ct [n, msg_size + 2, 12], inputs_rest [n, n_abc - 1 - msg_size, 4] canonical scalars (ignored
    when there are none), A [n,12], B [n,24], C [n,12] -> (verdict [n] uint8, 1 = accepted; reason [n] uint8: 0 accepted, 1 malformed,
    else 2 = the ciphertext equation fails | 4 = the Groth16 equation fails).  Exact per-ballot verdicts; the points are assumed to
    be in the subgroups (decode with check_subgroup)."""
    A = _u64(A, 12); B = _u64(B, 24); Cc = _u64(Cc, 12)
    n = A.shape[0]
    n_rest = ver.n_abc - 1 - ver.msg_size
    ct = _u64(ct).reshape(n, -1)
    rest = _u64(inputs_rest).reshape(n, -1) if n_rest else np.zeros((n, 4), np.uint64)
    if B.shape[0] != n or Cc.shape[0] != n or ct.shape[1] != 12 * (ver.msg_size + 2) or (n_rest and rest.shape[1] != 4 * n_rest):
        raise ValueError("saver_verify_batch: n ballots (ct[msg_size + 2, 12], A[12], B[24], C[12]) and n x (n_abc - 1 - msg_size) rest inputs expected")
    verdict = np.zeros(n, np.uint8); reason = np.zeros(n, np.uint8)
    ctx.check(ctx.lib.vsp_saver_verify_batch(ctx.h, ver.h, _ptr(ct), _ptr(rest), _ptr(A), _ptr(B), _ptr(Cc), n, _ptr(verdict), _ptr(reason)))
    return verdict, reason


def saver_verify_batch_screened(ctx, ver, ct, inputs_rest, A, B, Cc, coeff=None):
    """saver_verify_batch with the well-formed ballots of a range accepted together under one random linear combination
    (vsp_saver_verify_batch_screened): the same arguments and results; a verdict of 0 and its reason always come from the exact path.
    coeff [n, 2]: the little-endian 128-bit coefficients, none zero; None draws them from `secrets`.  They must be fresh, uniform and
    drawn after the ballots are fixed: then an invalid ballot of subgroup points is accepted with probability at most 1 / (2^128 - 1)."""
    A = _u64(A, 12); B = _u64(B, 24); Cc = _u64(Cc, 12)
    n = A.shape[0]
    n_rest = ver.n_abc - 1 - ver.msg_size
    ct = _u64(ct).reshape(n, -1)
    rest = _u64(inputs_rest).reshape(n, -1) if n_rest else np.zeros((n, 4), np.uint64)
    if coeff is None:
        zs = [secrets.randbelow((1 << 128) - 1) + 1 for _ in range(n)]
        coeff = np.array([[z & 0xFFFFFFFFFFFFFFFF, z >> 64] for z in zs], np.uint64).reshape(n, 2)
    coeff = _u64(coeff).reshape(-1, 2)
    if B.shape[0] != n or Cc.shape[0] != n or coeff.shape[0] != n or ct.shape[1] != 12 * (ver.msg_size + 2) or (n_rest and rest.shape[1] != 4 * n_rest):
        raise ValueError("saver_verify_batch_screened: n ballots (ct[msg_size + 2, 12], A[12], B[24], C[12]), n x (n_abc - 1 - msg_size) rest inputs and n x 2 coefficient words expected")
    verdict = np.zeros(n, np.uint8); reason = np.zeros(n, np.uint8)
    ctx.check(ctx.lib.vsp_saver_verify_batch_screened(ctx.h, ver.h, _ptr(ct), _ptr(rest), _ptr(A), _ptr(B), _ptr(Cc), n, _ptr(coeff), _ptr(verdict), _ptr(reason)))
    return verdict, reason


def saver_receive_blobs(ctx, ver, ct_blobs, proof_blobs, input_blobs, coeff=None, tally=None, check_subgroup=True):
    """The ballot box's receiving step (vsp_saver_receive_blobs): n ballots as their blobs -- ct_blobs n x (8 + 48 (msg_size + 2))
    bytes, proof_blobs n x 192, input_blobs n x (8 + 32 n_rest) scalar vectors of the remaining public inputs (None when there are
    none); each one bytes object or a list of per-ballot blobs.  Decodes every point once on the GPU, gives the verdicts of
    saver_verify_batch (coeff None) or saver_verify_batch_screened (coeff [n, 2], little-endian 128-bit words, none zero, fresh and
    drawn after the ballots are fixed) and adds exactly the accepted ballots to `tally` (a Tally of ct_len msg_size + 2, or None).
    Returns (verdict [n] uint8, reason [n] uint8, wire_status [n, 3] uint8: the bytes of Tally.add_blobs, proofs_from_blob_batch and
    0 / 1 for the input blob; accepted).  A ballot with a wire status byte set has verdict 0 and reason 1."""
    def joined(b):
        return bytes(b) if isinstance(b, (bytes, bytearray, memoryview)) else b"".join(bytes(x) for x in b)
    n_rest = ver.n_abc - 1 - ver.msg_size
    ct = joined(ct_blobs); pr = joined(proof_blobs); inp = None if input_blobs is None else joined(input_blobs)
    ct_size = 8 + 48 * (ver.msg_size + 2); in_size = 8 + 32 * n_rest
    if len(ct) % ct_size or len(pr) != len(ct) // ct_size * 192 or (inp is not None and len(inp) != len(ct) // ct_size * in_size) or (inp is None and n_rest):
        raise ValueError(f"saver_receive_blobs: n ciphertext blobs of {ct_size} bytes, n proofs of 192 bytes and n input blobs of {in_size} bytes expected")
    n = len(ct) // ct_size
    if coeff is not None:
        coeff = _u64(coeff).reshape(-1, 2)
        if coeff.shape[0] != n:
            raise ValueError("saver_receive_blobs: n x 2 coefficient words expected")
    verdict = np.zeros(n, np.uint8); reason = np.zeros(n, np.uint8); wire = np.zeros((n, 3), np.uint8); accepted = C.c_size_t(0)
    bufs = [np.frombuffer(b if b else bytes(1), dtype=np.uint8) if b is not None else None for b in (ct, pr, inp)]
    ctx.check(ctx.lib.vsp_saver_receive_blobs(ctx.h, ver.h, tally.h if tally is not None else None, _ptr(bufs[0]), _ptr(bufs[1]), _ptr(bufs[2]), n, int(check_subgroup),
                                              _ptr(coeff), _ptr(verdict), _ptr(reason), _ptr(wire), C.byref(accepted)))
    return verdict, reason, wire, accepted.value


FREE, FIXED, SERIAL = 0, 1, 2                                       # roles of a rest input in a BallotBox


class BallotBox:
    """A ballot box over a SaverVerifier (vsp_ballot_box): which serial numbers are spent, and whether a ballot's FIXED rest inputs are
    this election's, decided on the GPU.  roles [n_rest]: FREE, FIXED or SERIAL per rest input; expected [n_rest, 4]: the canonical
    scalars the FIXED inputs must equal (the other rows are ignored).  The reference's eid | sn | rt is (FIXED, SERIAL, FIXED).  The
    verifier must outlive the box.  Option "ballot_box_table_bits" is read at creation."""

    def __init__(self, ctx, ver, expected, roles):
        self.ctx, self.ver = ctx, ver
        role = np.ascontiguousarray(roles, dtype=np.uint8).reshape(-1)
        exp = _u64(expected, 4)
        if exp.shape[0] != role.shape[0]:
            raise ValueError("BallotBox: one role and one expected scalar per rest input")
        self.h = ctx.lib.vsp_ballot_box_create(ctx.h, ver.h, _ptr(exp), _ptr(role), role.shape[0])
        if not self.h:
            raise VspError("vsp_ballot_box_create failed: " + ctx.last_error())
        self.serial_scalars = ctx.lib.vsp_ballot_box_serial_scalars(self.h)

    def free(self):
        if self.h:
            self.ctx.lib.vsp_ballot_box_free(self.ctx.h, self.h)
            self.h = None

    def count(self):
        """ballots accepted so far: the next ordinal"""
        return self.ctx.lib.vsp_ballot_box_count(self.h)

    def device_bytes(self):
        return self.ctx.lib.vsp_ballot_box_device_bytes(self.h)

    def receive_blobs(self, ct_blobs, proof_blobs, input_blobs, coeff=None, tally=None, check_subgroup=True):
        """saver_receive_blobs with the box's rule (vsp_ballot_box_receive_blobs): a ballot is accepted when it is not wire-rejected, its
        FIXED inputs are the box's, the verifier accepts it and no earlier accepted ballot holds its serial.  Returns (verdict, reason,
        wire_status, accepted, holder [n] uint64): reason 8 = a FIXED input differs, 16 = the serial is spent, and then holder is the
        ordinal of the ballot that holds it (all-ones otherwise; a ballot the verifier refused, reason 2, 4 or 6, whose serial an earlier
        accepted ballot holds gets that ordinal too, so that holder does not depend on the piece boundaries)."""
        def joined(b):
            return bytes(b) if isinstance(b, (bytes, bytearray, memoryview)) else b"".join(bytes(x) for x in b)
        ver = self.ver
        n_rest = ver.n_abc - 1 - ver.msg_size
        ct = joined(ct_blobs); pr = joined(proof_blobs); inp = joined(input_blobs)
        ct_size = 8 + 48 * (ver.msg_size + 2); in_size = 8 + 32 * n_rest
        if len(ct) % ct_size or len(pr) != len(ct) // ct_size * 192 or len(inp) != len(ct) // ct_size * in_size:
            raise ValueError(f"BallotBox.receive_blobs: n ciphertext blobs of {ct_size} bytes, n proofs of 192 bytes and n input blobs of {in_size} bytes expected")
        n = len(ct) // ct_size
        if coeff is not None:
            coeff = _u64(coeff).reshape(-1, 2)
            if coeff.shape[0] != n:
                raise ValueError("BallotBox.receive_blobs: n x 2 coefficient words expected")
        verdict = np.zeros(n, np.uint8); reason = np.zeros(n, np.uint8); wire = np.zeros((n, 3), np.uint8); accepted = C.c_size_t(0)
        holder = np.full(n, 0xFFFFFFFFFFFFFFFF, np.uint64)
        bufs = [np.frombuffer(b if b else bytes(1), dtype=np.uint8) for b in (ct, pr, inp)]
        ctx = self.ctx
        ctx.check(ctx.lib.vsp_ballot_box_receive_blobs(ctx.h, self.h, tally.h if tally is not None else None, _ptr(bufs[0]), _ptr(bufs[1]), _ptr(bufs[2]), n,
                                                       int(check_subgroup), _ptr(coeff), _ptr(verdict), _ptr(reason), _ptr(wire), C.byref(accepted), _ptr(holder)))
        return verdict, reason, wire, accepted.value, holder

    def serials(self, first=0, count=None):
        """the serials of ordinals [first, first + count) as [count, S, 4] canonical scalars (count None: to the end)"""
        if count is None:
            count = self.count() - first
        out = np.zeros((max(count, 0), self.serial_scalars, 4), np.uint64)
        self.ctx.check(self.ctx.lib.vsp_ballot_box_serials(self.ctx.h, self.h, int(first), int(count), _ptr(out)))
        return out

    def add_serials(self, serials):
        """restore exported serials, or add serials in bulk: [count, S, 4]; the first occurrence wins and gets the next ordinal.  Returns
        (status [count] uint8, 1 = already held; added)"""
        s = _u64(serials).reshape(-1, self.serial_scalars, 4)
        status = np.zeros(s.shape[0], np.uint8); added = C.c_size_t(0)
        self.ctx.check(self.ctx.lib.vsp_ballot_box_add_serials(self.ctx.h, self.h, _ptr(s), s.shape[0], _ptr(status), C.byref(added)))
        return status, added.value


class Pedersen:
    """The Pedersen hash over Jubjub under the caller's generators (vsp_pedersen): generators [g, 8] canonical u | v, validated by the
    library (on the curve, of prime order, not the identity; equal generators are accepted), their window tables resident on the GPU.
    A message has 1 .. max_bits = 189 g bits."""

    def __init__(self, ctx, generators):
        self.ctx = ctx
        gens = _u64(generators, 8)
        h = C.c_void_p(None)
        ctx.check(ctx.lib.vsp_pedersen_create(ctx.h, _ptr(gens), gens.shape[0], C.byref(h)))
        self.h = h
        self.generators = ctx.lib.vsp_pedersen_generators(self.h)
        self.max_bits = ctx.lib.vsp_pedersen_max_bits(self.h)

    def free(self):
        if self.h:
            self.ctx.lib.vsp_pedersen_free(self.ctx.h, self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def device_bytes(self):
        return self.ctx.lib.vsp_pedersen_device_bytes(self.h)


def pedersen_hash_batch(ctx, ped, msgs, nbits, points=False):
    """count hashes of nbits bits each (vsp_pedersen_hash_batch): msgs [count, ceil(nbits / 64)] words, bit k of a message at word
    k // 64, position k % 64 (bits at or above nbits are ignored).  Returns the digests [count, 4] (the canonical u of the hash point,
    255 bits), and with points=True also the points [count, 8] (u | v)."""
    row = (int(nbits) + 63) // 64
    m = _u64(msgs, max(row, 1))
    digests = np.zeros((m.shape[0], 4), np.uint64)
    pts = np.zeros((m.shape[0], 8), np.uint64) if points else None
    ctx.check(ctx.lib.vsp_pedersen_hash_batch(ctx.h, ped.h, _ptr(m), int(nbits), m.shape[0], _ptr(digests), _ptr(pts)))
    return (digests, pts) if points else digests


def digest_scalars(digests):
    """digests [n, 4] of 255 bits as the circuit's public inputs [n, 2, 4]: the low 254 bits and the bit above them, the packing of
    get_multi_field_element_from_bits (common.hpp:563-574) that Registry.rt_scalars applies to the root.  Both scalars are below r, as a
    BallotBox expects its FIXED values and compares its serials"""
    d = _u64(digests, 4)
    out = np.zeros((d.shape[0], 2, 4), np.uint64)
    out[:, 0, :] = d
    out[:, 0, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
    out[:, 1, 0] = (d[:, 3] >> np.uint64(62)) & np.uint64(1)
    return out


class Registry:
    """The Merkle tree of the voters' public keys on the GPU (vsp_registry): arity 2, Pedersen hashes of `ped` (at least 3 generators),
    nodes of 255 bits, leaves first and the root last.  Made by Registry.build or Registry.from_blob."""

    def __init__(self, ctx, handle, first_bad_node=None):
        self.ctx, self.h = ctx, handle
        self.depth = ctx.lib.vsp_registry_depth(handle)
        self.first_bad_node = first_bad_node        # from_blob(verify=True): None when the tree is consistent, else the lowest node that differs

    @classmethod
    def build(cls, ctx, ped, pks, depth, hash_leaves=True):
        """the tree of depth `depth` over pks [count, 4] (255-bit keys, count <= 2^depth; absent keys are zero).  hash_leaves: level 0 is
        H(pk) (the default, a guess: DESIGN.md 3.6i) or pk itself"""
        keys = _u64(pks, 4)
        h = C.c_void_p(None)
        ctx.check(ctx.lib.vsp_registry_build(ctx.h, ped.h, _ptr(keys if keys.shape[0] else np.zeros((1, 4), np.uint64)), keys.shape[0], int(depth), int(bool(hash_leaves)),
                                             C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_blob(cls, ctx, ped, blob, depth, verify=True):
        """the tree of a blob of 32 (2^(depth + 1) - 1) octets; verify: every inner node is compared with the hash of its children on the
        GPU and first_bad_node names the lowest one that differs"""
        data = np.frombuffer(bytes(blob) if blob else bytes(1), dtype=np.uint8)
        h = C.c_void_p(None); bad = C.c_uint64(0)
        ctx.check(ctx.lib.vsp_registry_from_blob(ctx.h, ped.h, _ptr(data), len(blob), int(depth), int(bool(verify)), C.byref(h), C.byref(bad)))
        return cls(ctx, h, None if bad.value == 0xFFFFFFFFFFFFFFFF else bad.value)

    def free(self):
        if self.h:
            self.ctx.lib.vsp_registry_free(self.ctx.h, self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def device_bytes(self):
        return self.ctx.lib.vsp_registry_device_bytes(self.h)

    def root(self):
        out = np.zeros(4, np.uint64)
        self.ctx.check(self.ctx.lib.vsp_registry_root(self.ctx.h, self.h, _ptr(out), None))
        return out

    def rt_scalars(self):
        """rt as the circuit's two public inputs [2, 4]: root mod 2^254 and root >> 254"""
        root = np.zeros(4, np.uint64); out = np.zeros((2, 4), np.uint64)
        self.ctx.check(self.ctx.lib.vsp_registry_root(self.ctx.h, self.h, _ptr(root), _ptr(out)))
        return out

    def nodes(self, level, first=0, count=None):
        """nodes [first, first + count) of a level (0 = the leaves, depth = the root) as [count, 4]; count None: to the level's end"""
        if count is None:
            count = (1 << (self.depth - level)) - first
        out = np.zeros((max(count, 0), 4), np.uint64)
        self.ctx.check(self.ctx.lib.vsp_registry_nodes(self.ctx.h, self.h, int(level), int(first), int(count), _ptr(out if out.shape[0] else np.zeros((1, 4), np.uint64))))
        return out

    def paths(self, indices):
        """the copaths of leaf indices [n] as [n, depth, 4]: level l holds node(l, (x >> l) ^ 1)"""
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        out = np.zeros((idx.shape[0], self.depth, 4), np.uint64)
        dummy = np.zeros(4, np.uint64)
        self.ctx.check(self.ctx.lib.vsp_registry_paths(self.ctx.h, self.h, _ptr(idx if idx.shape[0] else dummy), idx.shape[0], _ptr(out if out.size else dummy)))
        return out

    def to_blob(self):
        out = np.zeros(self.ctx.lib.vsp_registry_blob_size(self.depth), np.uint8)
        self.ctx.check(self.ctx.lib.vsp_registry_to_blob(self.ctx.h, self.h, _ptr(out)))
        return out.tobytes()


class _BorrowedR1CS:
    """the constraint system a VoteCircuit owns, as every prover, generator and checker call takes one"""

    def __init__(self, ctx, handle, num_constraints, num_inputs, num_vars):
        self.ctx, self.h = ctx, handle
        self.num_constraints, self.num_inputs, self.num_vars = num_constraints, num_inputs, num_vars
        self.m = ctx.lib.vsp_r1cs_domain_size(handle)
        self.domain_kind = ("basic_radix2", "step_radix2")[ctx.lib.vsp_r1cs_domain_kind(handle)]

    check = R1CS.check
    check_device = R1CS.check_device
    is_satisfied = R1CS.is_satisfied

    def free(self):
        self.h = None


class VoteCircuit:
    """The voting circuit (vsp_vote_circuit): "I know sk and a copath such that H(sk) is a leaf of the tree with root rt,
    sn = H(eid | sk), and m is my ballot", built from the hash `ped` (which must outlive it).  Public inputs m_1 .. m_n | eid_packed |
    sn_packed (2) | rt_packed (2).  .cs is its constraint system for groth16 / saver calls; .blocks names the wires of a witness."""

    BLOCKS = ("M", "EID_PACKED", "SN_PACKED", "RT_PACKED", "EID_BITS", "SK_BITS", "ADDRESS_BITS", "COPATH_BITS", "SN_BITS", "RT_BITS")

    def __init__(self, ctx, ped, msg_size, eid_bits, depth, hash_leaves=True):
        self.ctx = ctx
        h = C.c_void_p(None)
        ctx.check(ctx.lib.vsp_vote_circuit_create(ctx.h, ped.h, int(msg_size), int(eid_bits), int(depth), int(bool(hash_leaves)), C.byref(h)))
        self.h = h
        self.msg_size, self.eid_bits, self.depth, self.hash_leaves = int(msg_size), int(eid_bits), int(depth), bool(hash_leaves)
        m, ni, nv = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        nnz = (C.c_size_t * 3)()
        ctx.check(ctx.lib.vsp_vote_circuit_sizes(self.h, C.byref(m), C.byref(ni), C.byref(nv), nnz))
        self.num_constraints, self.num_inputs, self.num_vars, self.nnz = m.value, ni.value, nv.value, [int(x) for x in nnz]
        self.cs = _BorrowedR1CS(ctx, ctx.lib.vsp_vote_circuit_r1cs(self.h), self.num_constraints, self.num_inputs, self.num_vars)
        self.blocks = {}
        for i, name in enumerate(self.BLOCKS):
            first, count = C.c_size_t(0), C.c_size_t(0)
            ctx.check(ctx.lib.vsp_vote_circuit_wires(self.h, i, C.byref(first), C.byref(count)))
            self.blocks[name] = (first.value, count.value)

    def free(self):
        if self.h:
            self.ctx.lib.vsp_vote_circuit_free(self.ctx.h, self.h)
            self.h = None
            self.cs.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def csr(self):
        """the three matrices as uploaded: [(row_ptr u32 [m + 1], col u32 [nnz], coef u64 [nnz, 4])] * 3, columns ascending in every row"""
        out = []
        for k in range(3):
            rp = np.zeros(self.num_constraints + 1, np.uint32); col = np.zeros(max(self.nnz[k], 1), np.uint32); coef = np.zeros((max(self.nnz[k], 1), 4), np.uint64)
            self.ctx.check(self.ctx.lib.vsp_vote_circuit_csr(self.h, k, _ptr(rp), _ptr(col), _ptr(coef)))
            out.append((rp, col[:self.nnz[k]], coef[:self.nnz[k]]))
        return out

    def _eid(self, eid_words):
        return _u64(eid_words, (self.eid_bits + 63) // 64).reshape(-1)

    def _members(self, sks, indices, votes):
        sks = _u64(sks, 4)
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        votes = np.ascontiguousarray(votes, dtype=np.uint32).reshape(-1)
        if not (sks.shape[0] == idx.shape[0] == votes.shape[0]):
            raise ValueError("VoteCircuit: sks, indices and votes must have one entry per ballot")
        return sks, idx, votes

    def witness_host(self, eid_words, sk, index, vote, copath):
        """one ballot's witness by the header's one-core host path from an explicit copath [depth, 4] (tests and measurements)
        -> (witness [num_vars, 4], leaf [4])"""
        out = np.zeros((self.num_vars, 4), np.uint64); leaf = np.zeros(4, np.uint64)
        cp = np.ascontiguousarray(copath, dtype=np.uint64).reshape(-1)
        rc = self.ctx.lib.vsp_vote_witness_host(self.h, _ptr(self._eid(eid_words)), _ptr(_u64(sk, 4).reshape(-1)), int(index), int(vote),
                                                _ptr(cp if cp.size else np.zeros(4, np.uint64)), _ptr(out), _ptr(leaf))
        if rc:
            raise ValueError("VoteCircuit.witness_host: vote, index or sk out of range")
        return out, leaf

    def witness_batch(self, reg, eid_words, sks, indices, votes):
        """the witnesses of count ballots on the GPU against a resident Registry (vsp_vote_witness_batch)
        -> (witnesses [count, num_vars, 4], status u8 [count]: 0 ok, 1 not the registry's leaf, 2 vote / index / sk out of range)"""
        sks, idx, votes = self._members(sks, indices, votes)
        n = sks.shape[0]
        wit = np.zeros((n, self.num_vars, 4), np.uint64); status = np.zeros(max(n, 1), np.uint8)
        dummy = np.zeros(4, np.uint64)
        self.ctx.check(self.ctx.lib.vsp_vote_witness_batch(self.ctx.h, self.h, reg.h, _ptr(self._eid(eid_words)), _ptr(sks if n else dummy), _ptr(idx if n else dummy),
                                                           _ptr(votes if n else np.zeros(1, np.uint32)), n, _ptr(wit if n else dummy), _ptr(status)))
        return wit, status[:n]

    def witness_batch_device(self, reg, eid_words, sks, indices, votes):
        """the witnesses of count (1..64) ballots left in the circuit's device buffer (vsp_cast_witness_batch_device)
        -> (device pointer, stride in values, status u8 [count]); member k is row k.  They stay until witness_release, the next witness
        or cast call on the circuit, or free."""
        sks, idx, votes = self._members(sks, indices, votes)
        n = sks.shape[0]
        d, stride = C.c_void_p(None), C.c_size_t(0)
        status = np.zeros(max(n, 1), np.uint8)
        self.ctx.check(self.ctx.lib.vsp_cast_witness_batch_device(self.ctx.h, self.h, reg.h, _ptr(self._eid(eid_words)), _ptr(sks), _ptr(idx), _ptr(votes), n,
                                                                  C.byref(d), C.byref(stride), _ptr(status)))
        return d.value, stride.value, status[:n]

    def witness_release(self):
        """zero the witnesses a device call left in the circuit's buffer, stream-ordered (vsp_cast_witness_release)"""
        self.ctx.check(self.ctx.lib.vsp_cast_witness_release(self.ctx.h, self.h))

    def cast_batch_launch(self, reg, spk, pk, eid_words, sks, indices, votes, r_enc, r, s):
        """first half of cast_batch on the device path (vsp_cast_batch_launch): blocks for the status words alone -> status u8 [count]"""
        sks, idx, votes = self._members(sks, indices, votes)
        K = sks.shape[0]
        rnd = [np.ascontiguousarray(x, dtype=np.uint64).reshape(K, 4) for x in (r_enc, r, s)]
        status = np.zeros(max(K, 1), np.uint8)
        self.ctx.check(self.ctx.lib.vsp_cast_batch_launch(self.ctx.h, self.h, reg.h, spk.h, pk.h, _ptr(self._eid(eid_words)), _ptr(sks), _ptr(idx), _ptr(votes), K,
                                                          _ptr(rnd[0]), _ptr(rnd[1]), _ptr(rnd[2]), _ptr(status)))
        self._cast = (K, status[:K])
        return status[:K]

    def cast_batch_finish(self):
        """second half (vsp_cast_batch_finish) -> as cast_batch"""
        K, status = getattr(self, "_cast", None) or (0, None)
        self._cast = None
        if not K:
            self.ctx.check(self.ctx.lib.vsp_cast_batch_finish(self.ctx.h, None, None, None, None, None, None))      # the library's refusal
            raise RuntimeError("cast_batch_finish: no batch launched through this circuit")
        n = self.msg_size
        ct = np.zeros((K, n + 2, 12), np.uint64)
        A = np.zeros((K, 12), np.uint64); B = np.zeros((K, 24), np.uint64); Cc = np.zeros((K, 12), np.uint64)
        proofs = np.zeros((K, 192), np.uint8); bl = np.zeros((K, self.ctx.lib.vsp_g1_vector_blob_size(n + 2)), np.uint8)
        rc = self.ctx.lib.vsp_cast_batch_finish(self.ctx.h, _ptr(ct), _ptr(A), _ptr(B), _ptr(Cc), _ptr(proofs), _ptr(bl))
        results = (ct, (A, B, Cc), [proofs[k].tobytes() for k in range(K)], [bl[k].tobytes() for k in range(K)], status)
        try:
            self.ctx.check(rc)
        except Unsatisfied as e:
            e.results = results
            raise
        return results

    def cast_batch(self, reg, spk, pk, eid_words, sks, indices, votes, r_enc, r, s):
        """count (1..64) ballots in one call (vsp_vote_cast_batch): the witnesses, then saver_encrypt_batch with m one-hot at the vote.
        With option vote_cast_device (default 1) the witnesses stay on the device; 0 sends them through host memory: the same outputs.
        -> (ct, (A, B, C), [proof bytes], [ciphertext blob bytes], status); a member of non-zero status has all-zero outputs"""
        sks, idx, votes = self._members(sks, indices, votes)
        K, n = sks.shape[0], self.msg_size
        rnd = [np.ascontiguousarray(x, dtype=np.uint64).reshape(K, 4) for x in (r_enc, r, s)]
        ct = np.zeros((K, n + 2, 12), np.uint64)
        A = np.zeros((K, 12), np.uint64); B = np.zeros((K, 24), np.uint64); Cc = np.zeros((K, 12), np.uint64)
        proofs = np.zeros((K, 192), np.uint8); bl = np.zeros((K, self.ctx.lib.vsp_g1_vector_blob_size(n + 2)), np.uint8)
        status = np.zeros(max(K, 1), np.uint8)
        rc = self.ctx.lib.vsp_vote_cast_batch(self.ctx.h, self.h, reg.h, spk.h, pk.h, _ptr(self._eid(eid_words)), _ptr(sks), _ptr(idx), _ptr(votes), K, _ptr(rnd[0]),
                                              _ptr(rnd[1]), _ptr(rnd[2]), _ptr(ct), _ptr(A), _ptr(B), _ptr(Cc), _ptr(proofs), _ptr(bl), _ptr(status))
        results = (ct, (A, B, Cc), [proofs[k].tobytes() for k in range(K)], [bl[k].tobytes() for k in range(K)], status[:K])
        try:
            self.ctx.check(rc)
        except Unsatisfied as e:
            e.results = results
            raise
        return results


class SaverDecryptor:
    """The opening side of a SAVER election resident on the GPU (vsp_saver_decryptor), made of public data only: the prepared
    Miller-loop lines of rho_sv_g2, rho_rhov_g2, H and -rho_g2, the bases e(G_i, rho_rhov_g2[i]) and their baby-step tables for
    messages in [0, max_value].  vk_words is the flat verification key of saver_generate_keypair, gamma_abc_g1 the first
    msg_size + 1 points of the accumulation vector.  baby_bits / fp_bits set the options "saver_decrypt_baby_bits" /
    "saver_decrypt_fp_bits" for this creation alone (None: the context's values); afterwards the options are what they were.  A context
    manager: the handle is freed on exit."""

    def __init__(self, ctx, vk_words, gamma_abc_g1, msg_size, max_value, baby_bits=None, fp_bits=None):
        self.ctx = ctx
        self.msg_size = int(msg_size)
        self.h = None
        words = _u64(vk_words).reshape(-1)
        gabc = _u64(gamma_abc_g1, 12)
        if self.msg_size < 1 or words.shape[0] != ctx.lib.vsp_saver_vk_words(self.msg_size) or gabc.shape[0] < self.msg_size + 1:
            raise ValueError("SaverDecryptor: vk_words / gamma_abc_g1 are not a verification key of this msg_size")
        if not 0 <= int(max_value) < 1 << 64:
            raise ValueError("SaverDecryptor: max_value outside 0 .. 2^64 - 1")
        # the two options are read at creation only: set for this creation, then put back to what they were (or their defaults)
        forced = {k: x for k, x in (("saver_decrypt_baby_bits", baby_bits), ("saver_decrypt_fp_bits", fp_bits)) if x is not None}
        before = {k: ctx.options.get(k, {"saver_decrypt_baby_bits": 0, "saver_decrypt_fp_bits": 64}[k]) for k in forced}
        try:
            for k, x in forced.items():
                ctx.set_option(k, x)
            self.h = ctx.lib.vsp_saver_decryptor_create(ctx.h, self.msg_size, _ptr(words), _ptr(gabc), int(max_value))
            err = ctx.last_error()
        finally:
            for k, x in before.items():
                ctx.set_option(k, x)
        if not self.h:
            raise VspError("vsp_saver_decryptor_create failed: " + err)
        self.max_value = ctx.lib.vsp_saver_decryptor_max_value(self.h)
        self.baby_bits = ctx.lib.vsp_saver_decryptor_baby_bits(self.h)

    def free(self):
        if self.h:
            self.ctx.lib.vsp_saver_decryptor_free(self.ctx.h, self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def base(self, slot):
        """e(G_{slot+1}, rho_rhov_g2[slot]) as 576 bytes"""
        gt = np.zeros(576, np.uint8)
        self.ctx.check(self.ctx.lib.vsp_saver_decryptor_base(self.h, int(slot), _ptr(gt)))
        return gt.tobytes()


def saver_decrypt_batch(ctx, dec, rho, ct):
    """decrypt of n ciphertexts (usually the one Tally.result()): rho [4] the secret key, ct [n, msg_size + 2, 12] ->
    (msgs [n, msg_size] uint64, nu [n, 12] the decryption proofs rho c_0, status [n, msg_size] uint8: 0 found, 1 no message in
    [0, max_value] (msgs is 2^64 - 1), 2 malformed ciphertext).  The points are assumed to be in the subgroup."""
    rho = _u64(rho).reshape(4)
    ct = _u64(ct).reshape(-1, 12 * (dec.msg_size + 2))
    n = ct.shape[0]
    msgs = np.zeros((n, dec.msg_size), np.uint64); nu = np.zeros((n, 12), np.uint64); status = np.zeros((n, dec.msg_size), np.uint8)
    if n:
        ctx.check(ctx.lib.vsp_saver_decrypt_batch(ctx.h, dec.h, _ptr(rho), _ptr(ct), n, _ptr(msgs), _ptr(nu), _ptr(status)))
    return msgs, nu, status


def saver_verify_decryption_batch(ctx, dec, ct, msgs, nu):
    """verify_decryption of n stated results: ct [n, msg_size + 2, 12], msgs [n, msg_size] python ints or uint64, or
    [n, msg_size, 4] canonical scalars, nu [n, 12] -> (verdict [n] uint8, 1 = accepted; reason [n] uint8: 0 accepted, 1 malformed,
    else 2 = the equation of nu fails | 4 = a slot equation fails; first_bad_slot [n] uint32, 2^32 - 1 when no slot fails)."""
    ct = _u64(ct).reshape(-1, 12 * (dec.msg_size + 2))
    n = ct.shape[0]
    m = np.asarray(msgs, dtype=object)      # Python objects first: no numeric coercion may touch an integer of up to 256 bits
    if m.size == n * dec.msg_size:
        m = np.array([[(int(x) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for x in m.reshape(-1)], dtype=np.uint64)
    else:
        m = np.array([int(x) for x in m.reshape(-1)], dtype=np.uint64)
    m = m.reshape(n, -1)
    nu = _u64(nu).reshape(-1, 12)
    if m.shape[1] != 4 * dec.msg_size or nu.shape[0] != n:
        raise ValueError("saver_verify_decryption_batch: n results (ct[msg_size + 2, 12], msgs[msg_size], nu[12]) expected")
    verdict = np.zeros(n, np.uint8); reason = np.zeros(n, np.uint8); first = np.full(n, 0xFFFFFFFF, np.uint32)
    if n:
        ctx.check(ctx.lib.vsp_saver_verify_decryption_batch(ctx.h, dec.h, _ptr(ct), _ptr(m), _ptr(nu), n, _ptr(verdict), _ptr(reason), _ptr(first)))
    return verdict, reason, first


# ---- wire formats (f.2): the big-endian blobs of the reference's marshaling_policy (common.hpp:168-203, 462-485, 749-799) ---------
def fr_vector_to_blob(vals):
    """serialize a scalar vector (primary input, eid, sn, rt, voting result): 8-byte count + 32-byte big-endian elements"""
    vals = _u64(vals, 4)
    out = np.zeros(_lib.load().vsp_fr_vector_blob_size(vals.shape[0]), np.uint8)
    if _lib.load().vsp_fr_vector_to_blob(_ptr(vals), vals.shape[0], _ptr(out)) != 0:
        raise ValueError("fr_vector_to_blob: value not canonical")
    return out.tobytes()


def fr_vector_from_blob(blob):
    """deserialize_scalar_vector (common.hpp:529-535)"""
    buf = np.frombuffer(bytes(blob), dtype=np.uint8); n = C.c_size_t(0)
    if _lib.load().vsp_fr_vector_from_blob(_ptr(buf), buf.shape[0], None, 0, C.byref(n)) != 0:
        raise ValueError("fr_vector_from_blob: malformed blob")
    out = np.zeros((n.value, 4), np.uint64)
    if _lib.load().vsp_fr_vector_from_blob(_ptr(buf), buf.shape[0], _ptr(out), n.value, C.byref(n)) != 0:
        raise ValueError("fr_vector_from_blob: element not canonical")
    return out


def g1_vector_to_blob(pts):
    """serialize the ciphertext (common.hpp:471-474): 8-byte count + compressed G1 points"""
    pts = _u64(pts, 12)
    out = np.zeros(_lib.load().vsp_g1_vector_blob_size(pts.shape[0]), np.uint8)
    if _lib.load().vsp_g1_vector_to_blob(_ptr(pts), pts.shape[0], _ptr(out)) != 0:
        raise ValueError("g1_vector_to_blob failed")
    return out.tobytes()


def g1_vector_from_blob(blob, check_subgroup=True):
    """deserialize_ct (common.hpp:773-781)"""
    buf = np.frombuffer(bytes(blob), dtype=np.uint8); n = C.c_size_t(0)
    if _lib.load().vsp_g1_vector_from_blob(_ptr(buf), buf.shape[0], int(check_subgroup), None, 0, C.byref(n)) != 0:
        raise ValueError("g1_vector_from_blob: malformed blob")
    out = np.zeros((n.value, 12), np.uint64)
    if _lib.load().vsp_g1_vector_from_blob(_ptr(buf), buf.shape[0], int(check_subgroup), _ptr(out), n.value, C.byref(n)) != 0:
        raise ValueError("g1_vector_from_blob: invalid point")
    return out


def proof_from_blob(blob, check_subgroup=True):
    buf = np.frombuffer(bytes(blob), dtype=np.uint8)
    if buf.shape[0] != 192:
        raise ValueError("proof_from_blob: a proof is 192 bytes")
    A = np.zeros(12, np.uint64); B = np.zeros(24, np.uint64); Cc = np.zeros(12, np.uint64)
    if _lib.load().vsp_proof_from_blob(_ptr(buf), int(check_subgroup), _ptr(A), _ptr(B), _ptr(Cc)) != 0:
        raise ValueError("proof_from_blob: invalid encoding")
    return A, B, Cc


def vk_to_blob(gt_bytes, gamma_g2, delta_g2, delta_g1, gamma_abc_g1, gamma_g1, head=0):
    """extended verification key; gt_bytes = alpha_g1_beta_g2 as 576 opaque bytes (12 little-endian Fp, computed by whoever has the pairing)"""
    gabc = _u64(gamma_abc_g1, 12); gt = np.frombuffer(bytes(gt_bytes), dtype=np.uint8)
    if gt.shape[0] != 576:
        raise ValueError("vk_to_blob: alpha_g1_beta_g2 is 576 bytes")
    out = np.zeros(_lib.load().vsp_vk_blob_size(gabc.shape[0]), np.uint8)
    if _lib.load().vsp_vk_to_blob(int(head), _ptr(gt), _ptr(_u64(gamma_g2)), _ptr(_u64(delta_g2)), _ptr(_u64(delta_g1)), _ptr(gabc), gabc.shape[0],
                                  _ptr(_u64(gamma_g1)), _ptr(out)) != 0:
        raise ValueError("vk_to_blob failed")
    return out.tobytes()


def vk_from_blob(blob, check_subgroup=True):
    buf = np.frombuffer(bytes(blob), dtype=np.uint8); n = C.c_size_t(0)
    lib = _lib.load()
    if lib.vsp_vk_from_blob(_ptr(buf), buf.shape[0], 0, None, None, None, None, None, None, 0, C.byref(n), None) != 0:
        raise ValueError("vk_from_blob: malformed blob")
    head = C.c_uint32(0); gt = np.zeros(576, np.uint8)
    g2 = np.zeros(24, np.uint64); d2 = np.zeros(24, np.uint64); d1 = np.zeros(12, np.uint64); g1 = np.zeros(12, np.uint64)
    gabc = np.zeros((n.value, 12), np.uint64)
    if lib.vsp_vk_from_blob(_ptr(buf), buf.shape[0], int(check_subgroup), C.byref(head), _ptr(gt), _ptr(g2), _ptr(d2), _ptr(d1), _ptr(gabc), n.value,
                            C.byref(n), _ptr(g1)) != 0:
        raise ValueError("vk_from_blob: invalid point")
    return dict(head=head.value, alpha_g1_beta_g2=gt.tobytes(), gamma_g2=g2, delta_g2=d2, delta_g1=d1, gamma_ABC_g1=gabc, gamma_g1=g1)
