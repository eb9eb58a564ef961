"""Decryption's exact rounding (csrc/encrypt.hip k_dec_round) restated word for word in Python integers, and PHASES crafted so that the
rounding, the noise bit length and the quotient j sit on their edges.  No GPU imports, no library: the reference is Python big integers
and nothing else.  tests/test_decrypt_craft_cpu.py proves the coverage conditions on the model, tests/test_gpu_decrypt_extremes.py runs
the same rows through fhe_decrypt_batch.

Specification, for a phase x in [0, q), q = prod q_i:
    m(x)     = ((t x + q // 2) // q) % t
    noise(x) = |t x - ((t x + q // 2) // q) q|
    figure of a ciphertext = max over its coefficients of noise.bit_length(); budget = max(0, q.bit_length() - figure - 1)

A size-2 ciphertext (c_0, c_1 = 0) has phase c_0 for EVERY secret key, so residue row i of c_0 is x mod q_i: phases are placed without
any key arithmetic.

Crafted families of one base (h = q // 2, t^-1 taken modulo q), at seeded scattered positions of one polynomial of n = 1024:
    ends        x in {0, 1, q - 1, h, h + 1}; x = q - 1 makes A + j wrap past t
    boundary    x(delta) = (delta - h) t^-1 mod q gives (t x + h) mod q = delta, delta = -8 .. 8: delta = 0 is the one value with
                M == j q exactly (the `>=` of big_ge at equality), delta = -1 is M == j q - 1
    noise       t x = s 2^b + e (mod q), s = +-1, e in {-1, 0, 1}: noise exactly |s 2^b + e| for every b in {0, 1, 31, 32, 62, 63, 64,
                65, 127, 128, 191, 192, ...} with 2^b < h -- every word boundary of the (k + 1)-word subtraction from both sides
    every j     the kernel's own r_i chosen directly (r_i = t y_i mod q_i is a bijection of phase_i): r_i = min(q_i - 1,
                floor(q_i a / (2k + 1))), a = 0 .. 2k + 1 (the last one is all r_i = q_i - 1)
    plain       the first and the last x with m = t - 1, the last x with m = 0 and the first with m = 1
    filler      seeded random x
The kernel reports ONE noise figure per ciphertext, a maximum over its n coefficients, and in such a row the filler (noise about q/2)
owns it.  So every value of the noise family, and +-h, comes a second time ALONE in a ciphertext whose other phases are 0 (`quiet`): its
figure is |v|.bit_length() and its budget q.bit_length() - figure - 1, positive below the top bit length.
"""
import functools
import random
from math import gcd

from galois_oracle import Q3, Q4
from ntt_craft import largest_primes
from packed_oracle import T41

N = 1024
M64 = (1 << 64) - 1
SEED = 20261
Q5 = Q4 + [0x7FFFFFFEAC0001]                                  # + the third 55-bit prime of the SEAL23_16384 preset
DELTAS = tuple(range(-8, 9))

# (base, k, t): every K = 1 .. 8 of k_dec_round<K>, prime widths 33 / 36-37 / 54-55 / 58 / 61 bits, t from 257 to the 2^60 refusal
CASES = ([("W61", k, t) for k in (1, 2, 8) for t in ((1 << 60) - 1, (1 << 59) + 1)]
         + [("W58", k, t) for k in (6, 7) for t in (T41, 65537)]
         + [("Q4", k, t) for k in (3, 4, 5) for t in (65537, 1 << 14)]
         + [("Q3", k, 12289) for k in (2, 3)] + [("W33", 2, 257)])
WIDTHS = [("W61", 2, (1 << 59) + 1), ("W58", 6, T41), ("Q4", 3, 65537), ("Q3", 2, 12289), ("W33", 2, 257)]      # one case per prime width


def primes(name, k):
    if name == "W61":
        return largest_primes(61, N, k)
    if name == "W58":
        return largest_primes(58, N, k)
    if name == "W33":
        return largest_primes(33, N, k)
    return list({"Q4": Q5, "Q3": Q3}[name][:k])


def product(q):
    out = 1
    for p in q:
        out *= p
    return out


# ---- the specification -------------------------------------------------------------------------------------------------------------------
def plain_of(x, Q, t):
    return ((t * x + Q // 2) // Q) % t


def noise_of(x, Q, t):
    return abs(t * x - ((t * x + Q // 2) // Q) * Q)


def budget_of(bits, Q):
    return max(0, Q.bit_length() - bits - 1)


# ---- the kernel's constants (fhe_decrypt_batch: DecConsts) and k_dec_round, word for word ---------------------------------------------------
def words(v, L):
    assert 0 <= v < 1 << (64 * L), "a multi-word value does not fit its %d words" % L
    return [(v >> (64 * l)) & M64 for l in range(L)]


def unwords(w):
    return sum(v << (64 * l) for l, v in enumerate(w))


def clz64(v):
    assert 0 < v <= M64
    return 64 - v.bit_length()


class Consts:
    def __init__(self, q, t):
        self.q, self.t, self.k, self.L = list(q), t, len(q), len(q) + 1
        self.Q = product(q)
        self.punct = [self.Q // p for p in q]
        self.inv_punct = [pow(P % p, -1, p) for P, p in zip(self.punct, q)]
        self.t_mod_q = [t % p for p in q]
        self.qinv64 = []
        for p in q:                                             # Newton: q^-1 mod 2^64 for odd q
            inv = p
            for _ in range(6):
                inv = inv * (2 - p * inv) & M64
            assert inv * p & M64 == 1
            self.qinv64.append(inv)
        self.punct_w = [words(P, self.L) for P in self.punct]
        self.jq = [words(j * self.Q, self.L) for j in range(self.k + 1)]
        self.qhalf = words(self.Q // 2, self.L)


def big_ge(a, b, gt=False):
    """from the least significant word up: the last difference decides; gt: the deliberately wrong `>` (equality answers false)"""
    ge = not gt
    for x, y in zip(a, b):
        if x != y:
            ge = x > y
    return ge


def round_model(res, C, gt=False, drop_c2=False, clz_prev=False):
    """k_dec_round on the phase residues of ONE coefficient -> (plaintext, noise bit length, j).  Every u64 register is kept below 2^64
    as the kernel keeps it; the assertions are the kernel's unstated preconditions (a < t, no carry out of the top word).
    Deliberately wrong variants: gt (`>` for `>=` in big_ge), drop_c2 (carry = hi + c1), clz_prev (64 - clz taken from the word BEFORE
    the borrow is applied, d1, in the place of d2)."""
    t, L = C.t, C.L
    Nw, A = [0] * L, 0
    for i, p in enumerate(C.q):
        assert 0 <= res[i] < p
        y = res[i] * C.inv_punct[i] % p                         # mul_barrett: canonical
        r = C.t_mod_q[i] * y % p
        a = ((t * y - r) & M64) * C.qinv64[i] & M64
        assert a < t and a * p + r == t * y, "the exact division by q_i through q_i^-1 mod 2^64"
        A += a
        if A >= t:
            A -= t
        carry = 0
        for l in range(L):                                      # N += r * punct_i
            prod = r * C.punct_w[i][l]
            lo, hi = prod & M64, prod >> 64
            s1 = (Nw[l] + lo) & M64
            c1 = int(s1 < lo)
            s2 = (s1 + carry) & M64
            c2 = int(s2 < carry)
            Nw[l] = s2
            carry = hi + c1 + (0 if drop_c2 else c2)
            assert carry <= M64
        assert carry == 0 or drop_c2, "sum_i r_i (q/q_i) left its k + 1 words"
    Mw, cy = [0] * L, 0
    for l in range(L):                                          # M = N + floor(q/2)
        s1 = (Nw[l] + C.qhalf[l]) & M64
        c1 = int(s1 < Nw[l])
        s2 = (s1 + cy) & M64
        c2 = int(s2 < cy)
        Mw[l] = s2
        cy = c1 + c2
    assert cy == 0 or drop_c2, "N + floor(q/2) left its k + 1 words"
    j = sum(1 for m in range(1, C.k + 1) if big_ge(Mw, C.jq[m], gt))
    v = A + j
    while v >= t:
        v -= t
    J = C.jq[j]
    pos = big_ge(Nw, J, gt)
    borrow, bits = 0, 0
    for l in range(L):
        hi_, lo_ = (Nw[l], J[l]) if pos else (J[l], Nw[l])
        d1, b1 = (hi_ - lo_) & M64, int(hi_ < lo_)
        d2, b2 = (d1 - borrow) & M64, int(d1 < borrow)
        borrow = b1 + b2
        if d2:
            bits = 64 * l + 64 - clz64(d1 if clz_prev and d1 else d2)
    return v, bits, j


# ---- crafted phases ------------------------------------------------------------------------------------------------------------------------
def noise_exponents(h):
    out = [0, 1, 31, 32, 62, 63, 64, 65]
    w = 2
    while (1 << (64 * w - 1)) < h:
        out += [64 * w - 1, 64 * w]
        w += 1
    return [b for b in out if (1 << b) < h]


def plain_modulus(q, t):
    """a listed t that is not coprime to q gives way to the next odd value below it (t is below every prime: fhe_ctx_create refuses otherwise)"""
    assert t < min(q)
    Q = product(q)
    while gcd(t, Q) != 1:
        t = t - 1 if t % 2 == 0 else t - 2
    return t


class Crafted:
    """one base: q, t, Q, consts; x[n] the phases; where[(family, label)] = coefficient index; want_plain[n], want_noise[n] from the big-integer
    formula; model[n] = (plain, bits, j) from round_model; residues() = the uint64 rows [k][n] of c_0"""

    def residues(self, x=None):
        import numpy as np
        x = self.x if x is None else x
        return np.array([[v % p for v in x] for p in self.q], dtype=np.uint64)

    def bits(self, x=None):
        return max(noise_of(v, self.Q, self.t).bit_length() for v in (self.x if x is None else x))

    def with_noise(self, v):
        """the phase whose t x is v modulo q: invariant noise exactly |v| for |v| <= h"""
        assert abs(v) <= self.Q // 2
        return v * self.tinv % self.Q


@functools.lru_cache(maxsize=None)
def craft(name, k, t, n=N, seed=SEED):
    q = primes(name, k)
    t = plain_modulus(q, t)
    cr = Crafted()
    cr.name, cr.q, cr.k, cr.t, cr.n = name, q, k, t, n
    cr.C = C = Consts(q, t)
    cr.Q = Q = C.Q
    h = Q // 2
    cr.tinv = tinv = pow(t, -1, Q)
    vals = [(("ends", lab), x) for lab, x in (("0", 0), ("1", 1), ("q-1", Q - 1), ("h", h), ("h+1", h + 1))]
    vals += [(("boundary", d), (d - h) * tinv % Q) for d in DELTAS]
    for b in noise_exponents(h):
        for s in (1, -1):
            for e in (-1, 0, 1):
                vals.append((("noise", (b, s, e)), (s * (1 << b) + e) * tinv % Q))
    for a in range(2 * k + 2):
        r = [min(p - 1, p * a // (2 * k + 1)) for p in q]
        vals.append((("every j", a), sum(ri * P for ri, P in zip(r, C.punct)) % Q * tinv % Q))
    first_top = -(-((t - 1) * Q - h) // t)                       # the smallest x with t x + h >= (t - 1) q
    vals += [(("plain", "first t-1"), first_top), (("plain", "last t-1"), (t * Q - h - 1) // t),
             (("plain", "last 0"), (Q - h - 1) // t), (("plain", "first 1"), -(-(Q - h) // t))]
    rng = random.Random("decrypt/%s/%d/%d/%d" % (name, k, t, seed))
    assert len(vals) <= n // 2
    cr.x = [rng.randrange(Q) for _ in range(n)]
    cr.where = {}
    for (key, x), pos in zip(vals, rng.sample(range(n), len(vals))):
        assert 0 <= x < Q
        cr.x[pos], cr.where[key] = x, pos
    cr.filler = sorted(set(range(n)) - set(cr.where.values()))
    # the noise family again, each value ALONE in a ciphertext of zero phases: the kernel reports one figure per ciphertext, a maximum over
    # its n coefficients, and in the row above the filler (noise about q/2) owns it.  (label, signed noise v, coefficient index)
    quiet = [((b, s, e), s * (1 << b) + e) for b in noise_exponents(h) for s in (1, -1) for e in (-1, 0, 1)] + [("h", h), ("-h", -h)]
    cr.quiet = [(lab, v, rng.randrange(n)) for lab, v in quiet]
    cr.want_plain = [plain_of(x, Q, t) for x in cr.x]
    cr.want_noise = [noise_of(x, Q, t) for x in cr.x]
    cr.model = [round_model([x % p for p in q], C) for x in cr.x]
    return cr
