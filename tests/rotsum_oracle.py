"""Specification of the hoisted special-prime rotations (include/fhe_hip.h: fhe_rotate_sum_sp / fhe_rotate_each_sp), restated on the
UNCHANGED CPU oracle: only Oracle.ntt_fwd / ntt_inv per prime, Python-integer slot products, tests/modswitch_oracle.py's drop and
tests/galois_oracle.py's sigma.  Nothing here calls the library.

The setting is tests/keyswitch_sp_oracle.py's: k primes, L = k - 1, p = q_(k-1) the special prime, ciphertexts [2][L][n], keys [L][2][k][n].
Taps (g_j, w_j, K_j), g_j odd in [1, 2n) and pairwise distinct, g = 1 "no rotation, no key"; w'_j the centred lift of w_j mod t.
  D_i,r    = NTT_(q_r)([c_1,i]_(q_r))
  pi_g     = the slot permutation with pi_g(NTT(a)) = NTT(sigma_g(a)); from the transform of X: slot s holds psi^(e_s) and reads the slot
             that holds psi^(e_s g)
  acc_pp,r = sum_(j: g_j != 1) w'_j sum_i pi_(g_j)(D_i,r) (*) K_j,i,pp,r mod q_r,   u_pp = one drop (k -> k - 1) of acc_pp
  sum:       (u_0 + sum_j w'_j sigma_(g_j)(c_0),  u_1 + sum_(j: g_j = 1) w'_j c_1)
  each:      out[j] = (sigma_(g_j)(c_0) + u_0^(j), u_1^(j)) with tap j alone and w' = 1; the input itself for g_j = 1
The digit of tap j is sigma_g(d_i) over the integers, coefficients in (-q_i, q_i): rotate_sum_big says so in big integers.  It is NOT
keyswitch_sp_oracle.apply_galois's digit (negated modulo q_i, then reduced): accumulator_difference states the difference.
Three forms: residues on the oracle's transforms (the GPU tests' reference), big integers through CRT modulo Q p (small n), and a model
of the kernels' lazy tap sum in 64-bit registers, with the WRONG variants the crafted operands are there to catch."""
import numpy as np

import galois_oracle as go
import keyswitch_sp_oracle as ks
import modswitch_oracle as mo

VARIANTS = ("perm_inv", "uncentred", "no_id_c1", "neg_q0")
MAX_TAPS = 64
FOLD_TAPS = 32                      # csrc/rotsum.hip RS_FOLD_TAPS


def _obj(a):
    return np.array([int(x) for x in a], dtype=object)


def _u64(a):
    return np.array([int(x) for x in a], dtype=np.uint64)


def centred(w, t):
    """the centred lift of w mod t, in (-t/2, t/2]"""
    w = int(w) % t
    return w - t if 2 * w > t else w


def check_taps(n, t, k, elts, weights):
    """the refusals of fhe_rotsum_plan_create that need no device: the reason, or None"""
    if k < 2:
        return "at least 2 primes"
    if not 1 <= len(elts) <= MAX_TAPS:
        return "tap count"
    if len(weights) != len(elts):
        return "one weight per tap"
    for j, g in enumerate(elts):
        if not (g & 1) or not 0 < g < 2 * n:
            return "Galois element %d: must be odd" % g
        if g in elts[:j]:
            return "Galois element %d is repeated" % g
        if int(weights[j]) % t == 0:
            return "weight of tap %d is 0 modulo t" % j
    return None


_perm = {}


def slot_perm(orc, g, r=0):
    """[n] int: pi_g reads slot s from slot perm[s], derived from the oracle's own transform of X modulo q_r"""
    key = (id(orc), g, r)
    if key not in _perm:
        n, q = orc.n, orc.q[r]
        x = np.zeros(n, dtype=np.uint64)
        x[1] = 1
        xh = [int(v) for v in orc.ntt_fwd(x, r)]
        where = {v: s for s, v in enumerate(xh)}
        assert len(where) == n
        _perm[key] = np.array([where[pow(v, g, q)] for v in xh], dtype=np.int64)
    return _perm[key]


def _sigma1(a, g, q):
    return np.asarray(a, dtype=np.uint64).copy() if g == 1 else go.sigma(a, g, q)


def _sigma_neg_other(v, g, qr, qo):
    """sigma_g of one residue polynomial modulo q_r with the WRONG negation (q_o - x) mod q_r"""
    n = len(v)
    e = np.arange(n, dtype=np.int64) * g % (2 * n)
    v = _obj(v)
    out = np.zeros(n, dtype=object)
    out[e % n] = np.where(e >= n, np.array([(qo - x) % qr if x else 0 for x in v], dtype=object), v)
    return out


# ---- the residue form on the oracle's transforms ------------------------------------------------------------------------------------------
def digits(orc, c1):
    """D [k][L][n] object arrays: D[r][i] = NTT_(q_r)([c_1,i]_(q_r)) in the oracle's slot order"""
    k, q = orc.k, orc.q
    return [[_obj(orc.ntt_fwd(np.asarray(c1[i], dtype=np.uint64) % np.uint64(q[r]), r)) for i in range(k - 1)] for r in range(k)]


def accumulators(orc, D, elts, wc, keys, variant=None):
    """acc [2][k][n] canonical COEFFICIENTS: sum over the taps with g != 1 of w'_j sum_i pi_(g_j)(D_i,r) (*) K_j,i,pp,r; wc: the centred weights"""
    k, n, q = orc.k, orc.n, orc.q
    acc = np.zeros((2, k, n), dtype=np.uint64)
    for r in range(k):
        for pp in range(2):
            s = np.zeros(n, dtype=object)
            for g, w, key in zip(elts, wc, keys):
                if g == 1:
                    continue
                perm = slot_perm(orc, pow(g, -1, 2 * n) if variant == "perm_inv" else g, r)
                s = (s + w * sum(D[r][i][perm] * _obj(key[i, pp, r]) for i in range(k - 1))) % q[r]
            acc[pp, r] = orc.ntt_inv(_u64(s), r)
    return acc


def _drop(acc, q):
    return np.stack([mo.switch_residues_levels(acc[pp], q)[len(q) - 1] for pp in range(2)])


def rotate_sum(orc, ct, t, elts, weights, keys, variant=None, D=None):
    """ct [2][L][n]; elts, weights [G]; keys [G]: [L][2][k][n] in the oracle's NTT form (anything for g = 1) -> [2][L][n]"""
    ct = np.asarray(ct, dtype=np.uint64)
    k, n, q = orc.k, orc.n, orc.q
    L = k - 1
    assert ct.shape == (2, L, n) and check_taps(n, t, k, list(elts), list(weights)) is None
    wc = [int(w) % t if variant == "uncentred" else centred(w, t) for w in weights]
    u = _drop(accumulators(orc, digits(orc, ct[1]) if D is None else D, elts, wc, keys, variant), q)
    out = np.zeros_like(ct)
    for r in range(L):
        s0, s1 = _obj(u[0, r]), _obj(u[1, r])
        for g, w in zip(elts, wc):
            if variant == "neg_q0" and g != 1:                           # sigma's negation modulo q_0 where q_r is meant (differs for r != 0)
                sg = _sigma_neg_other(ct[0, r], g, q[r], q[0])
            else:
                sg = _obj(_sigma1(ct[0, r][None], g, [q[r]])[0])
            s0 = (s0 + w * sg) % q[r]
            if g == 1 and variant != "no_id_c1":
                s1 = (s1 + w * _obj(ct[1, r])) % q[r]
        out[0, r], out[1, r] = _u64(s0), _u64(s1)
    return out


def rotate_each(orc, ct, t, elts, keys):
    """-> [G][2][L][n]"""
    ct = np.asarray(ct, dtype=np.uint64)
    D = digits(orc, ct[1])
    return np.stack([ct.copy() if g == 1 else rotate_sum(orc, ct, t, [g], [1], [key], D=D) for g, key in zip(elts, keys)])


def op_by_op_accumulators(orc, ct, g, key):
    """acc [2][k][n] of keyswitch_sp_oracle.apply_galois (negation modulo q_i, then the reduction), coefficient form"""
    k, n, q = orc.k, orc.n, orc.q
    d = go.sigma(ct, g, q[:-1])[1]
    acc = np.zeros((2, k, n), dtype=np.uint64)
    for r in range(k):
        D = [_obj(orc.ntt_fwd(d[i] % np.uint64(q[r]), r)) for i in range(k - 1)]
        for pp in range(2):
            acc[pp, r] = orc.ntt_inv(_u64(sum(D[i] * _obj(key[i, pp, r]) for i in range(k - 1)) % q[r]), r)
    return acc


def accumulator_difference(orc, ct, g, key):
    """what op-by-op's accumulators hold above the hoisted ones: sum_i (q_i mod q_r) M_i (*) K_i,pp,r, M_i the 0/1 mask of the coefficients of
    sigma_g(c_1,i) that are negated and non-zero.  [2][k][n], coefficient form"""
    k, n, q = orc.k, orc.n, orc.q
    e = np.arange(n, dtype=np.int64) * g % (2 * n)
    acc = np.zeros((2, k, n), dtype=np.uint64)
    for r in range(k):
        M = []
        for i in range(k - 1):
            mask = np.zeros(n, dtype=np.uint64)
            mask[e % n] = ((e >= n) & (np.asarray(ct[1, i]) != 0)).astype(np.uint64)
            M.append(_obj(orc.ntt_fwd(mask, r)))
        for pp in range(2):
            acc[pp, r] = orc.ntt_inv(_u64(sum((q[i] % q[r]) * M[i] * _obj(key[i, pp, r]) for i in range(k - 1)) % q[r]), r)
    return acc


# ---- big integers through CRT --------------------------------------------------------------------------------------------------------------
def sigma_signed(poly, g):
    """sigma_g over the integers: the digit of the hoisted key switch, coefficients in (-q_i, q_i)"""
    n = len(poly)
    out = [0] * n
    for j, v in enumerate(poly):
        e = j * g % (2 * n)
        out[e % n] = -int(v) if e >= n else int(v)
    return out


def rotate_sum_composed(q, t, c, elts, weights, K):
    """c [2][n] integers modulo Q; K [G]: [L][2][n] integers modulo Q p (None for g = 1) -> [2][n] integers modulo Q: the digits
    sigma_g(d_i) over Z, ONE rounding division by p of the weighted sum, then the additions modulo Q"""
    L, n = len(q) - 1, len(c[0])
    Qp, Q = mo.prod(q), mo.prod(q[:-1])
    wc = [centred(w, t) for w in weights]
    acc = [[0] * n, [0] * n]
    for g, w, Kj in zip(elts, wc, K):
        if g == 1:
            continue
        for i in range(L):
            d = [v % Qp for v in sigma_signed([x % q[i] for x in c[1]], g)]
            for pp in range(2):
                acc[pp] = [(x + w * y) % Qp for x, y in zip(acc[pp], mo.negacyclic_mul(d, Kj[i][pp], Qp))]
    out = [[mo.drop_big(v, q) for v in acc[pp]] for pp in range(2)]
    for g, w in zip(elts, wc):
        s0 = c[0] if g == 1 else ks.sigma_big(c[0], g, Q)
        out[0] = [(x + w * y) % Q for x, y in zip(out[0], s0)]
        if g == 1:
            out[1] = [(x + w * y) % Q for x, y in zip(out[1], c[1])]
    return out


def rotate_sum_big(q, t, ct, elts, weights, keys_coeff):
    """the same from residues (small n): K_j,i,pp composed modulo Q p from the coefficient-form keys -> residues [2][L][n]"""
    k, L = len(q), len(q) - 1
    n = np.asarray(ct).shape[-1]
    K = [None if g == 1 else [[[mo.compose([int(kc[i, pp, r, x]) for r in range(k)], q) for x in range(n)] for pp in range(2)] for i in range(L)]
         for g, kc in zip(elts, keys_coeff)]
    c = [[mo.compose([int(ct[pp][r][x]) for r in range(L)], q[:-1]) for x in range(n)] for pp in range(2)]
    out = rotate_sum_composed(q, t, c, elts, weights, K)
    return np.array([[[v % qi for v in out[pp]] for qi in q[:-1]] for pp in range(2)], dtype=np.uint64)


# ---- the lazy tap sum of csrc/rotsum.hip in 64-bit registers ---------------------------------------------------------------------------------
def tap_sum_bound_model(taps, rq16, q, fold_every=FOLD_TAPS, folded16=17):
    """the same sum with every term AT the bound the kernel's static_assert reasons with (rq16 / 16 q: the figure fhe_build_base checks
    mulvv_pm's result against, PmA.RQ = 96, PmB.RQ = 24) and every folded value at folded16 / 16 q: the largest register, through u64()"""
    from test_pm_arithmetic_model import u64
    s, since, top = 0, 0, 0
    for _ in range(taps):
        s = u64(s + rq16 * q // 16)
        top = max(top, s)
        since += 1
        if fold_every and since == fold_every:
            s, since = folded16 * q // 16, 0
    return top


def tap_sum_model(terms, m, fold_every=FOLD_TAPS):
    """terms: per tap ([(digit, key residue)] * L, w'_j mod q) of ONE slot of k_rs_accum_pm.  Every register goes through u64(): the L lazy
    products of a tap, their fold, the lazy product with the weight, the sum over taps folded every `fold_every` taps (None: never -- the
    WRONG variant), the last fold.  Returns (the folded value, the largest register seen)"""
    from test_pm_arithmetic_model import fold_pm, mulvv_pm, u64
    s, since, top = 0, 0, 0
    for pairs, w in terms:
        a = 0
        for x, e in pairs:
            a = u64(a + mulvv_pm(x, e, m))
        s = u64(s + mulvv_pm(fold_pm(a, m), w, m))
        top = max(top, s)
        since += 1
        if fold_every and since == fold_every:
            s, since = fold_pm(s, m), 0
    return fold_pm(s, m), top


# ---- crafted operands -----------------------------------------------------------------------------------------------------------------------
def edge_weights(t):
    return [1, t - 1, (t - 1) // 2, (t + 1) // 2]


class TapEdge:
    """family U of tests/keyswitch_sp_oracle.py (constant sources q_i - 1: digit a_i,r = (q_i - 1) mod q_r in every slot, whatever the slot
    order or the rotation), extended over taps of weight +-(t - 1)/2: per weight and prime r, eight tuples of key residues (e_0 .. e_(L-1))
    for which, in csrc/rotsum.hip's arithmetic, the product of the folded digit sum with w'_r is at or above q_r (tau + q_r, tau < delta:
    the top of what mulvv_pm returns for a weight this small): every term of the lazy tap sum is above q_r.  e_1 .. are Uniform's (every
    digit product above q_r); e_0 is solved for: sum_i a_i e_i = tau w'^-1 mod q_r with tau small, kept when the lazy product is tau + q_r.
    The general path computes canonically; its bytes must be the same."""

    def __init__(self, q, n, t, want=8):
        from test_pm_arithmetic_model import Pm, fold_pm, mulvv_pm
        self.q, self.n, self.k, self.L, self.t = list(q), n, len(q), len(q) - 1, t
        self.U = ks.Uniform(q, n, pm=True)
        self.weights = [(t - 1) // 2, (t + 1) // 2]
        self.res = {}
        for b, w in enumerate(self.weights):
            for r, qr in enumerate(q):
                m = Pm(qr)
                wr = centred(w, t) % qr
                a = [self.U.a[i][r] for i in range(self.L)]
                inv0, invw = pow(a[0], -1, qr), pow(wr, -1, qr)
                found, tau = [], 1
                while len(found) < want:
                    rest = [self.U.res[(i, r)][(len(found) + i) % 8] for i in range(1, self.L)]
                    e0 = (tau * invw - sum(x * e for x, e in zip(a[1:], rest))) % qr * inv0 % qr
                    es = [e0] + rest
                    lazy = mulvv_pm(fold_pm(sum(mulvv_pm(x, e, m) for x, e in zip(a, es)), m), wr, m)
                    assert lazy % qr == tau % qr
                    if lazy >= qr:
                        found.append(tuple(es))
                    tau += 1
                    assert tau < 100000, "no residues whose weighted lazy product is above q"
                self.res[(b, r)] = found

    def source(self):
        return self.U.source()

    def key(self, b):
        """[L][2][k][n] in NTT form for a tap of weight self.weights[b]: slot s of (pp, r) holds tuple (s + 5 pp) mod 8"""
        key = np.zeros((self.L, 2, self.k, self.n), dtype=np.uint64)
        slots = np.arange(self.n)
        for r in range(self.k):
            for pp in range(2):
                for i in range(self.L):
                    e = np.array([tp[i] for tp in self.res[(b, r)]], dtype=np.uint64)
                    key[i, pp, r] = e[(slots + 5 * pp) % len(e)]
        return key

    def key_coeff(self, orc, b):
        """the key whose ORACLE NTT form is key(b) (Uniform.key_coeff: each side transforms it into its own slot order)"""
        key = self.key(b)
        out = np.zeros_like(key)
        for idx in np.ndindex(key.shape[:2]):
            for r in range(self.k):
                out[idx + (r,)] = orc.ntt_inv(key[idx + (r,)], r)
        return out

    def slot_terms(self, r, taps, s=0, pp=0):
        """the terms of tap_sum_model for slot s of prime r: taps alternate the two weights"""
        out = []
        for j in range(taps):
            b = j & 1
            es = self.res[(b, r)][(s + 5 * pp) % 8]
            out.append(([(self.U.a[i][r], es[i]) for i in range(self.L)], centred(self.weights[b], self.t) % self.q[r]))
        return out


def filter_elements(n, tile_w, kw, kh):
    """the Galois elements of a kw x kh filter's taps over tiles of width tile_w, row-major with x fastest (circuits.packed_filter2d);
    the centre tap is g = 1"""
    ax, ay = (kw - 1) // 2, (kh - 1) // 2
    out = []
    for p in range(kw * kh):
        j, i = divmod(p, kw)
        steps = ((j - ay) * tile_w + (i - ax)) % (n // 2)
        out.append(pow(3, steps, 2 * n))
    return out


def many_elements(n, count):
    """`count` pairwise distinct elements, none of them 1: 3^1, 3^2, .."""
    out = [pow(3, j, 2 * n) for j in range(1, count + 1)]
    assert len(set(out)) == count and 1 not in out
    return out
