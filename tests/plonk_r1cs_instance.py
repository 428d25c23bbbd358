"""Circuits for the compile of a circom .r1cs to PLONK (include/zkhip.h, section "PLONK from an R1CS"): a generator of
satisfiable circuits of given shapes, a pure-Python compile written from the header's layout (vectors, maps, sigma, the
extension tables, extend), and check(), which tests a compiled circuit against a witness without knowing how it was made."""
import collections
import functools
import random

from oracle.bn254 import R_MOD as R, fr_root
from oracle.groth16_ref import write_wtns
from rapidsnark_old_amd import r1cs as r1cs_mod

K1, K2 = 2, 3
MIN_LOG_N = 3
TWICE = "zk_plonk_r1cs_create: constraint %d: %s names wire 0 twice"


# ---------------------------------------------------------------- the generator
class Builder:
    """Wires: 0 the constant, 1 .. n_public the publics, then n_free - n_public more inputs, all drawn; every constraint adds
    one fresh wire that solves its C (unless C is empty, which needs (A.w)(B.w) = 0)."""

    def __init__(self, seed, n_public, n_free):
        assert n_public <= n_free
        self.rng = random.Random(seed)
        self.n_public = n_public
        self.w = [1] + [self.rng.randrange(1, R) for _ in range(n_free)]
        self.n_inputs = 1 + n_free
        self.A, self.B, self.C = [], [], []

    def coef(self):
        return self.rng.choice((1, R - 1, 2, self.rng.randrange(1, R)))

    def lc(self, t, const=None, wires=None):
        """t terms on input wires (not wire 0), in drawn order; const: a term on wire 0 in a drawn place"""
        terms = [((wires[i] if wires else self.rng.randrange(1, self.n_inputs)), self.coef()) for i in range(t)]
        if const is not None:
            terms.insert(self.rng.randrange(len(terms) + 1), (0, const))
        return terms

    def value(self, lc):
        return sum(c * self.w[i] for i, c in lc) % R

    def add(self, A, B, C=(), c_coef=1, c_empty=False, fresh_first=False):
        """the constraint A * B = C + c_coef * fresh, the fresh wire set so that it holds; c_empty: A * B = C as given, no fresh wire"""
        prod = self.value(A) * self.value(B) % R
        C = list(C)
        if c_empty:
            assert prod == self.value(C)
        else:
            fresh = len(self.w)
            self.w.append((prod - self.value(C)) * pow(c_coef, -1, R) % R)
            C = [(fresh, c_coef)] + C if fresh_first else C + [(fresh, c_coef)]
        self.A.append(list(A)), self.B.append(list(B)), self.C.append(C)
        return len(self.w) - 1

    def unused_wire(self):
        self.w.append(self.rng.randrange(1, R))
        return len(self.w) - 1

    def done(self):
        data = r1cs_mod.write_r1cs_rows(self.A, self.B, self.C, len(self.w), self.n_public)
        return Case(data, list(self.w), self.n_public)


Case = collections.namedtuple("Case", "data witness n_public")
Case.wtns = property(lambda self: write_wtns(self.witness))
Case.publics = property(lambda self: self.witness[1:1 + self.n_public])


def _simple(b, count):
    for _ in range(count):
        b.add(b.lc(1), b.lc(1))


def _one_constraint(seed):                                  # three 1-term LCs, nPublic 0: N = 1, n = 8
    b = Builder(seed, 0, 2)
    b.add(b.lc(1), b.lc(1))
    return b.done()


def _empties(seed):                                         # empty A, empty B, empty C (and all three at once)
    b = Builder(seed, 2, 5)
    b.add([], b.lc(2))
    b.add(b.lc(1), [])
    b.add([], b.lc(1), c_empty=True)
    b.add([], [], c_empty=True)
    b.add(b.lc(3), [], C=[(0, 0)], c_empty=True)              # a C that is one dropped term
    return b.done()


def _constants(seed):                                       # an LC that is only a constant; a constant plus terms; a constant in C
    b = Builder(seed, 2, 6)
    b.add([(0, 7)], b.lc(1))
    b.add(b.lc(1), [(0, R - 1)])
    b.add([(0, 5)], [(0, 9)])
    b.add(b.lc(2, const=11), b.lc(1, const=3))
    b.add(b.lc(1, const=4), b.lc(3, const=R - 2), C=b.lc(2, const=13))
    b.add(b.lc(1), b.lc(1), C=[(0, 21)], fresh_first=True)
    b.add([(0, 6)], [(0, 7)], C=[(0, 42)], c_empty=True)       # 6 * 7 = 42: no wire at all
    return b.done()


def _zero_coefficients(seed):                               # zero coefficients that must be dropped, wire 0's among them
    b = Builder(seed, 2, 6)
    b.add([(3, 0), (4, 5), (2, 0)], [(0, 0), (1, 2), (5, 0), (6, 3)])
    b.add([(0, 0), (0, 4), (1, 1)], [(2, 0)], C=[(3, 0)], c_empty=True)
    b.add([(1, 0)], b.lc(2), C=[(2, 0)], c_empty=True)
    b.add(b.lc(2) + [(5, 0)], b.lc(1), C=[(4, 0), (3, 9), (0, 0)])
    return b.done()


def _chains(seed):                                          # t = 2 and t = 3 in each of A, B and C
    b = Builder(seed, 2, 8)
    for t in (2, 3):
        b.add(b.lc(t), b.lc(1))
        b.add(b.lc(1), b.lc(t))
        b.add(b.lc(1), b.lc(1), C=b.lc(t - 1))
        b.add(b.lc(t), b.lc(t), C=b.lc(t - 1), c_coef=R - 3, fresh_first=True)
    b.add(b.lc(5, const=2), b.lc(4), C=b.lc(6, const=1))
    return b.done()


def _same_wire_twice(seed):                                 # the same non-zero wire twice in one LC is two terms
    b = Builder(seed, 1, 4)
    b.add([(2, 3), (2, 5)], [(3, 1), (1, 2), (3, R - 1)])
    b.add(b.lc(1), b.lc(1), C=[(4, 2), (4, 2), (4, R - 4)])
    return b.done()


def _long_row(seed, t=1000):                                # one t-term row in A beside 1-term rows
    b = Builder(seed, 2, 40)
    _simple(b, 3)
    b.add(b.lc(t), b.lc(1))
    _simple(b, 3)
    return b.done()


def _rows(seed, n_rows, n_public=0):                        # N = n_rows exactly: 1-term LCs, one row a constraint
    b = Builder(seed, n_public, 4)
    _simple(b, n_rows - n_public)
    return b.done()


def _all_inputs_public(seed):
    b = Builder(seed, 5, 5)
    b.add(b.lc(2), b.lc(2))
    b.add(b.lc(1, const=1), b.lc(3))
    return b.done()


def _wire_in_all_columns(seed):                             # wire 3 in a, b and c; wire 5 named by no cell
    b = Builder(seed, 2, 5)
    b.add([(3, 2)], [(0, 3)], C=[(3, 6)], c_empty=True)       # 2 w3 * 3 = 6 w3: wire 3 is the final gate's a and c
    b.add([(3, 2)], [(3, 3)], C=[(3, 5)])
    b.add([(3, 1), (4, 1)], [(1, 1)], C=[(3, 1), (2, 1)])
    b.add([(1, 1)], [(3, 7)])
    b.unused_wire()
    b.add([(2, 1)], [(4, 1)])
    return b.done()


def _wide(seed, log_n=17):                                  # n_witness above 2^16; wire 0 in the first and the last row; no padding
    b = Builder(seed, 0, 50)
    m = 1 << log_n
    b.add(b.lc(1), [])
    for i in range(m - 2):
        b.add([(b.rng.randrange(1, len(b.w)), 1)], [(1 + i % 50, 2)])
    b.add([], b.lc(1), c_empty=True)
    return b.done()


def _proof(seed, log_n):                                    # N just below 2^log_n, every kind of row
    b = Builder(seed, 2, 6)
    target = (1 << log_n) - 1
    rows = 2
    while rows + 9 <= target:
        b.add(b.lc(3, const=5), b.lc(2), C=b.lc(2))          # 2 + 1 + 2 additions and the final gate: 6 rows
        b.add(b.lc(1), [(0, 3)])
        b.add(b.lc(2), b.lc(1, const=1))                   # 1 addition: 2 rows
        rows += 9
    _simple(b, target - rows)
    return b.done()


SHAPES = {
    "one_constraint": lambda: _one_constraint(7101),
    "empties": lambda: _empties(7102),
    "constants": lambda: _constants(7103),
    "zero_coefficients": lambda: _zero_coefficients(7104),
    "chains": lambda: _chains(7105),
    "same_wire_twice": lambda: _same_wire_twice(7106),
    "long_row": lambda: _long_row(7107),
    "rows_16": lambda: _rows(7108, 16),
    "rows_17": lambda: _rows(7109, 17),
    "rows_16_public_2": lambda: _rows(7110, 16, 2),
    "all_inputs_public": lambda: _all_inputs_public(7111),
    "wire_in_all_columns": lambda: _wire_in_all_columns(7112),
    "proof_3": lambda: _proof(7203, 3),
    "proof_4": lambda: _proof(7204, 4),
    "proof_6": lambda: _proof(7206, 6),
    "proof_8": lambda: _proof(7208, 8),
}
WIDE = "wide"                                                # compile only: 2^17 rows


@functools.lru_cache(maxsize=None)
def case(name):
    return _wide(7117) if name == WIDE else SHAPES[name]()


# ---------------------------------------------------------------- the compile, from the header's layout
Compiled = collections.namedtuple("Compiled", "log_n n rows n_public n_wires n_additions n_witness vectors maps ext k1 k2")
Compiled.__doc__ = """vectors: ql qr qm qo qc s1 s2 s3, n ints each (values over the domain); maps: a, b, c, n wire indices each; ext: a row an
addition gate, (wire, coefficient, chain_start, head_wire, head_coefficient): the head is the LC's first term, where a chain starts."""


def normalise(lc, j, name):
    kept = [(i, c % R) for i, c in lc if c % R]
    consts = [c for i, c in kept if i == 0]
    if len(consts) > 1:
        raise ValueError(TWICE % (j, name))
    return (consts[0] if consts else 0), [(i, c) for i, c in kept if i != 0]


def expected_rows(data):
    """(N, n_additions) by the header's formula"""
    h, cons = r1cs_mod.read_constraints(data)
    adds = sum(max(len(normalise(lc, j, "ABC"[k])[1]) - 1, 0) for j, lcs in enumerate(cons) for k, lc in enumerate(lcs))
    return h.nPublic + adds + len(cons), adds


@functools.lru_cache(maxsize=None)
def compile_r1cs(data, k1=K1, k2=K2):
    h, cons = r1cs_mod.read_constraints(data)
    n_public, n_wires = h.nPublic, h.nWires
    gates, ext = [], []                                     # a gate: (a, b, c, ql, qr, qm, qo, qc)
    for i in range(n_public):
        gates.append((1 + i, 0, 0, 1, 0, 0, 0, 0))
    for j, lcs in enumerate(cons):
        norm = [normalise(lc, j, "ABC"[k]) for k, lc in enumerate(lcs)]   # A before B before C
        reduced = []
        for k_l, terms in norm:
            if not terms:
                reduced.append((0, 0))
            elif len(terms) == 1:
                reduced.append(terms[0])
            else:
                for r in range(1, len(terms)):
                    new = n_wires + len(ext)
                    wire, c = terms[r]
                    if r == 1:
                        gates.append((terms[0][0], wire, new, terms[0][1], c, 0, R - 1, 0))
                        ext.append((wire, c, True, terms[0][0], terms[0][1]))
                    else:
                        gates.append((new - 1, wire, new, 1, c, 0, R - 1, 0))
                        ext.append((wire, c, False, 0, 0))
                reduced.append((n_wires + len(ext) - 1, 1))
        (ka, _), (kb, _), (kc, _) = norm
        (sa, ca), (sb, cb), (sc, cc) = reduced
        gates.append((sa, sb, sc, ca * kb % R, ka * cb % R, ca * cb % R, (R - cc) % R, (ka * kb - kc) % R))
    N = len(gates)
    log_n = max(MIN_LOG_N, (N - 1).bit_length())
    n = 1 << log_n
    gates += [(0,) * 8] * (n - N)
    maps = [[g[k] for g in gates] for k in range(3)]
    ql, qr, qm, qo, qc = ([g[k] for g in gates] for k in range(3, 8))
    # sigma: the cells of a wire in ascending index form one cycle
    by_wire = collections.defaultdict(list)
    for col in range(3):
        for row in range(n):
            by_wire[maps[col][row]].append(col * n + row)
    nxt = [0] * (3 * n)
    for cells in by_wire.values():
        for a, b in zip(cells, cells[1:] + cells[:1]):
            nxt[a] = b
    w, pw = fr_root(log_n), [1] * n
    for i in range(1, n):
        pw[i] = pw[i - 1] * w % R
    K = (1, k1, k2)
    sig = [K[t // n] * pw[t % n] % R for t in nxt]
    vectors = [ql, qr, qm, qo, qc, sig[:n], sig[n:2 * n], sig[2 * n:]]
    return Compiled(log_n, n, N, n_public, n_wires, len(ext), n_wires + len(ext), vectors, maps, ext, k1, k2)


def extend(c, witness):
    """the n_witness values: the circom witness and the running sums of the chains"""
    assert len(witness) == c.n_wires
    w = list(witness)
    acc = 0
    for wire, coef, start, hw, hc in c.ext:
        acc = (hc * w[hw] if start else acc) + coef * w[wire]
        acc %= R
        w.append(acc)
    return w


# ---------------------------------------------------------------- the check
def check(c, w_ext, publics):
    """None, or what is wrong first: a gate that does not hold (PI included), sigma not a permutation of the 3n cells, or
    its cycles not exactly the wire classes in ascending order"""
    n = c.n
    ql, qr, qm, qo, qc, s1, s2, s3 = c.vectors
    if len(w_ext) != c.n_witness or len(publics) != c.n_public:
        return "lengths"
    for i in range(n):
        a, b, cc = (w_ext[m[i]] for m in c.maps)
        pi = (R - publics[i]) % R if i < c.n_public else 0
        if (ql[i] * a + qr[i] * b + qm[i] * a * b + qo[i] * cc + qc[i] + pi) % R:
            return "gate %d" % i
    w, x = fr_root(c.log_n), 1
    cell_of = {}
    for row in range(n):
        for col, k in enumerate((1, c.k1, c.k2)):
            cell_of[k * x % R] = col * n + row
        x = x * w % R
    if len(cell_of) != 3 * n:
        return "the cosets overlap"
    sig = list(s1) + list(s2) + list(s3)
    nxt = [cell_of.get(v) for v in sig]
    if None in nxt or len(set(nxt)) != 3 * n:
        return "sigma is not a permutation of the cells"
    by_wire = collections.defaultdict(list)
    for cell in range(3 * n):
        by_wire[c.maps[cell // n][cell % n]].append(cell)
    for wire in sorted(by_wire):
        cells = by_wire[wire]
        for a, b in zip(cells, cells[1:] + cells[:1]):
            if nxt[a] != b:
                return "the cycle of wire %d" % wire
    return None
