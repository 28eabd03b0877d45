"""Big-integer judge of the voting circuit and the protocol's values of its public inputs.  Test infrastructure beside jubjub_model.py,
written from the definitions of the issue / DESIGN.md 3.3d alone: it knows nothing of the circuit's layout.

    Judge(A, B, C)          A z o B z = C z over an exported CSR (row_ptr, col, coef as words), z = (1, witness)
    public_inputs(...)      m one-hot | eid_packed | sn_packed | rt_packed for a voter, from jubjub_model's hash and tree
"""
import jubjub_model as jm

R = jm.R
PACK = 254


def from_words(w):
    return sum(int(x) << (64 * i) for i, x in enumerate(w))


class Judge:
    def __init__(self, A, B, C):
        """each matrix: (row_ptr [m + 1], col [nnz], coef [nnz, 4])"""
        self.m = len(A[0]) - 1
        self.mats = []
        for row_ptr, col, coef in (A, B, C):
            assert len(row_ptr) == self.m + 1
            rp = [int(x) for x in row_ptr]
            cols = [int(x) for x in col]
            vals = [from_words(c) for c in coef]
            assert all(v < R for v in vals)
            self.mats.append((rp, cols, vals))

    def failing_rows(self, witness):
        """the rows that z = (1, witness) fails; witness: integers (one per variable)"""
        z = [1] + [int(w) for w in witness]
        bad = []
        for r in range(self.m):
            dots = []
            for rp, cols, vals in self.mats:
                acc = 0
                for i in range(rp[r], rp[r + 1]):
                    acc += vals[i] * z[cols[i]]
                dots.append(acc % R)
            if dots[0] * dots[1] % R != dots[2]:
                bad.append(r)
        return bad

    def satisfied(self, witness):
        return all(0 <= int(w) < R for w in witness) and not self.failing_rows(witness)


def witness_ints(words):
    """[num_vars, 4] words -> integers"""
    return [from_words(row) for row in words]


def pack(bits):
    """bits -> scalars of 254 bits each: bit i goes to scalar i // 254 with weight 2^(i % 254)"""
    out = [0] * ((len(bits) + PACK - 1) // PACK)
    for i, b in enumerate(bits):
        out[i // PACK] += b << (i % PACK)
    return out


def serial_number(table, eid_bits, sk):
    """sn = H(eid | sk): the digest u as an integer"""
    return table.hash(list(eid_bits) + jm.bits_of(sk, jm.DIGEST_BITS))


def public_key(table, sk):
    return table.hash(jm.bits_of(sk, jm.DIGEST_BITS))


def public_inputs(table, n, eid_bits, sk, vote, root):
    """the public inputs of a ballot in the reference's order: m_1 .. m_n | eid_packed | sn_packed (2) | rt_packed (2)"""
    m = [1 if i == vote else 0 for i in range(n)]
    sn = serial_number(table, eid_bits, sk)
    return m + pack(list(eid_bits)) + pack(jm.bits_of(sn, jm.DIGEST_BITS)) + pack(jm.bits_of(root, jm.DIGEST_BITS))
