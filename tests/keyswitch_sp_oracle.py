"""Specification of the key switch with a special prime (include/fhe_hip.h: fhe_relinearize_sp_poly / fhe_apply_galois_sp), restated on
the UNCHANGED CPU oracle: only Oracle.ntt_fwd / ntt_inv per prime, Python-integer slot products, tests/modswitch_oracle.py's drop and
tests/galois_oracle.py's sigma.  Nothing here calls the library.

The context has k primes q_0 .. q_(k-1); L = k - 1, Q = q_0 .. q_(L-1), p = q_(k-1) is the special prime.  Ciphertexts are [size][L][n].
  key for a target T [k][n]:   [L][2][k][n], entry i = (-(a_i s + e_i) + P_i T, a_i); "+ P_i T" adds (p mod q_i) T mod q_i on component i only
  KS(d, K), d [L][n]:          acc_pp,r = sum_(i < L) [d_i]_(q_r) (*) K_i,pp,r mod q_r for r < k;  u_pp = one drop (k -> k - 1) of acc_pp
  relinearise step:            (c_0 + u_0, c_1 + u_1),        u = KS(c_src_poly, key for s^src_poly)
  Galois:                      (sigma_g(c_0) + u_0, u_1),     u = KS(sigma_g(c_1), key for sigma_g(s))
Three forms: residues on the oracle's transforms (the GPU tests' reference), big integers through CRT modulo Q p (small n), and a
per-coefficient / per-slot model of the kernels' arithmetic with the WRONG variants the crafted operands are there to catch."""
import numpy as np

import galois_oracle as go
import modswitch_oracle as mo

VARIANTS = ("gt_final", "neg0", "raw_d", "p_everywhere", "neg_qr")


def _obj(a):
    return np.array([int(x) for x in a], dtype=object)


def _u64(a):
    return np.array([int(x) for x in a], dtype=np.uint64)


def sigma_inverse(n, g):
    return pow(g, -1, 2 * n)


# ---- keys ------------------------------------------------------------------------------------------------------------------------------
def switch_key(orc, sk, target, seed=1, noise=3, variant=None):
    """[L][2][k][n] in COEFFICIENT form (each side transforms it into its own slot order): a test key for `target` [k][n] under the secret
    sk [k][n] (residues over all k primes), a uniform, e uniform in [-noise, noise].  variant "p_everywhere": the WRONG key that adds
    P_i T on every component r instead of component i only."""
    rng = np.random.default_rng(seed)
    k, n, q = orc.k, orc.n, orc.q
    p = q[-1]
    S = [_obj(orc.ntt_fwd(sk[r], r)) for r in range(k)]
    key = np.zeros((k - 1, 2, k, n), dtype=np.uint64)
    for i in range(k - 1):
        e = rng.integers(-noise, noise + 1, size=n)
        for r in range(k):
            qr = q[r]
            a = rng.integers(0, qr, size=n, dtype=np.uint64)
            a_s = _obj(orc.ntt_inv(_u64(_obj(orc.ntt_fwd(a, r)) * S[r] % qr), r))
            k0 = (-(a_s + _obj(e))) % qr
            if r == i or variant == "p_everywhere":
                k0 = (k0 + (p % qr) * _obj(target[r])) % qr
            key[i, 0, r], key[i, 1, r] = _u64(k0), a
    return key


def key_to_oracle(orc, key_coeff):
    """a key in coefficient form [.., k, n] in the oracle's NTT form"""
    key_coeff = np.asarray(key_coeff, dtype=np.uint64)
    out = np.zeros_like(key_coeff)
    for idx in np.ndindex(key_coeff.shape[:-2]):
        for r in range(orc.k):
            out[idx + (r,)] = orc.ntt_fwd(key_coeff[idx + (r,)], r)
    return out


def secret_powers(orc, sk, count):
    """[count][k][n]: s^2 .. s^(count+1) as residues over all k primes"""
    out, S = [], [_obj(orc.ntt_fwd(sk[r], r)) for r in range(orc.k)]
    cur = [s.copy() for s in S]
    for _ in range(count):
        cur = [c * s % qr for c, s, qr in zip(cur, S, orc.q)]
        out.append(np.stack([orc.ntt_inv(_u64(c), r) for r, c in enumerate(cur)]))
    return np.stack(out)


# ---- the residue form on the oracle's transforms ------------------------------------------------------------------------------------------
def key_switch(orc, d, key):
    """d [L][n] canonical coefficients, key [L][2][k][n] in the oracle's NTT form -> u [2][L][n]"""
    k, n, q = orc.k, orc.n, orc.q
    L = k - 1
    d = np.asarray(d, dtype=np.uint64)
    assert d.shape == (L, n) and key.shape == (L, 2, k, n)
    acc = np.zeros((2, k, n), dtype=np.uint64)
    for r in range(k):
        D = [_obj(orc.ntt_fwd(d[i] % np.uint64(q[r]), r)) for i in range(L)]          # [d_i]_(q_r): not centred
        for pp in range(2):
            s = sum(D[i] * _obj(key[i, pp, r]) for i in range(L)) % q[r]
            acc[pp, r] = orc.ntt_inv(_u64(s), r)
    return np.stack([mo.switch_residues_levels(acc[pp], q)[L] for pp in range(2)])


def _addmod(a, b, q):
    out = np.zeros_like(a)
    for r, qr in enumerate(q):
        out[..., r, :] = (a[..., r, :] + b[..., r, :]) % np.uint64(qr)                 # both below 2^61
    return out


def relinearize_poly(orc, ct, src_poly, key):
    """ct [size][L][n], size > src_poly >= 2 -> [2][L][n]"""
    ct = np.asarray(ct, dtype=np.uint64)
    assert src_poly >= 2 and ct.shape[0] > src_poly
    return _addmod(ct[:2], key_switch(orc, ct[src_poly], key), orc.q[:-1])


def relinearize(orc, ct, keys):
    """any size >= 3 down to 2, top polynomial first; keys [size - 2][L][2][k][n] for s^2 .."""
    cur = np.asarray(ct, dtype=np.uint64).copy()
    for p in range(cur.shape[0] - 1, 1, -1):
        cur[:2] = relinearize_poly(orc, cur, p, keys[p - 2])
    return cur[:2].copy()


def apply_galois(orc, ct, g, key):
    """ct [2][L][n] -> (sigma_g(c_0) + u_0, u_1)"""
    ct = np.asarray(ct, dtype=np.uint64)
    assert ct.shape == (2, orc.k - 1, orc.n)
    qL = orc.q[:-1]
    s = go.sigma(ct, g, qL)
    u = key_switch(orc, s[1], key)
    return np.stack([_addmod(s[0][None], u[0][None], qL)[0], u[1]])


# ---- big integers through CRT --------------------------------------------------------------------------------------------------------------
def key_switch_big(q, d, key_coeff):
    """the same on big integers (small n): K_i,pp composed modulo Q p from the coefficient-form key, acc_pp = sum_i D_i (*) K_i,pp mod Q p
    with D_i the integer polynomial of the residues d_i in [0, q_i), u_pp = floor((acc_pp + floor(p / 2)) / p) mod Q -> residues [2][L][n]"""
    k, L = len(q), len(q) - 1
    n = key_coeff.shape[-1]
    K = [[[mo.compose([int(key_coeff[i, pp, r, c]) for r in range(k)], q) for c in range(n)] for pp in range(2)] for i in range(L)]
    u = key_switch_composed(q, d, K)
    return np.array([[[v % qi for v in u[pp]] for qi in q[:-1]] for pp in range(2)], dtype=np.uint64)


def key_switch_composed(q, d, K):
    """K [L][2][n] integers modulo Q p, d [L][n] residues -> u [2][n] integers in [0, Q)"""
    L, n, Qp = len(q) - 1, len(K[0][0]), mo.prod(q)
    out = []
    for pp in range(2):
        acc = [0] * n
        for i in range(L):
            term = mo.negacyclic_mul([int(x) for x in d[i]], K[i][pp], Qp)
            acc = [(x + y) % Qp for x, y in zip(acc, term)]
        out.append([mo.drop_big(v, q) for v in acc])
    return out


def sigma_big(poly, g, qi):
    """sigma_g of one residue polynomial in Python integers"""
    n = len(poly)
    out = [0] * n
    for j, v in enumerate(poly):
        e = j * g % (2 * n)
        out[e % n] = (qi - v) % qi if e >= n else v
    return out


# ---- the kernels' arithmetic, one coefficient / slot at a time, with its wrong variants -----------------------------------------------------
def load_model(v, negated, qi, qr, variant=None):
    """[d_i]_(q_r) of a stored coefficient v of residue i that sigma_g negates (or not): negation modulo the SOURCE prime, the negation of 0
    is 0, then the reduction to q_r.  Variants: "neg0" (the negation of 0 gives q_i), "neg_qr" (the negation is taken modulo q_r),
    "raw_d" (d_i used as it is, without the reduction: the value a transform modulo q_r would take as if it were below q_r)."""
    if negated:
        if variant == "neg_qr":
            v = (qr - v % qr) % qr
        elif variant == "neg0":
            v = qi - v
        else:
            v = qi - v if v else 0
    return v if variant == "raw_d" else v % qr


def drop_model(x, cp, q, r, variant=None):
    """the drop of the special prime on one coefficient as csrc/keyswitch_sp.hip's ksp_drop has it (modswitch_oracle.switch_model for one kept
    prime): variant "gt_final" has `>` for `>=` in the last conditional subtraction"""
    return mo.switch_model([x, cp], [q[r], q[-1]], 1, variant="gt_final" if variant == "gt_final" else None)[0]


# ---- crafted operands -----------------------------------------------------------------------------------------------------------------------
def reduction_values(q, i):
    """family R, residue i: 0, 1, q_i - 1 and q_r - 1, q_r, q_r + 1, 2 q_r for every other prime r (the special one included) wherever they
    are below q_i"""
    qi = q[i]
    vals = [0, 1, qi - 1]
    for r, qr in enumerate(q):
        if r != i:
            vals += [v for v in (qr - 1, qr, qr + 1, 2 * qr) if v < qi]
    return sorted(set(vals))


def reduction_poly(q, n, g=None):
    """[L][n]: coefficient j of residue i holds value j mod len(values_i) of reduction_values -- twice over: first as stored, then (from
    position len(values_i) on, interleaved) as the value sigma_g turns INTO it where sigma_g negates the position (q_i - v).  g=None: a
    relinearisation source, nothing is negated."""
    L = len(q) - 1
    out = np.zeros((L, n), dtype=np.uint64)
    neg = (np.arange(n, dtype=np.int64) * g % (2 * n)) >= n if g is not None else np.zeros(n, dtype=bool)
    for i in range(L):
        vals = reduction_values(q, i)
        for j in range(n):
            v = vals[(j // 2 if g is not None else j) % len(vals)]
            if g is not None and (j & 1) and neg[j]:
                v = (q[i] - v) % q[i]                                   # the stored value whose negation is v
            out[i, j] = v
    return out


def drop_key_rows(orc, tiles):
    """family D: key row 0 as DATA, the oracle-form transform of tiles [2][k][n] (modswitch_oracle.crafted_tile of the base, one per output
    polynomial) in COEFFICIENT form = the tiles themselves; the other rows zero.  With d = the constant 1 on residue 0 and 0 elsewhere,
    acc_pp IS tiles[pp]."""
    key = np.zeros((orc.k - 1, 2, orc.k, orc.n), dtype=np.uint64)
    key[0] = tiles
    return key


def drop_tiles(q, n):
    return np.stack([mo.crafted_tile(q, len(q) - 1, n, seed=pp) for pp in range(2)])


def unit_source(q, n):
    d = np.zeros((len(q) - 1, n), dtype=np.uint64)
    d[0, 0] = 1
    return d


def final_addends(u, q):
    """[.., L, n] addends for the final addmod, per coefficient in turn: 0, q_r - 1, the complement that makes the sum exactly q_r (result 0)
    and the one that makes it q_r - 1; u: what the key switch adds"""
    u = np.asarray(u, dtype=np.uint64)
    out = np.zeros_like(u)
    j = np.arange(u.shape[-1])
    for r, qr in enumerate(q[:u.shape[-2]]):
        qr = np.uint64(qr)
        a = u[..., r, :]
        out[..., r, :] = np.where(j % 4 == 0, np.uint64(0), np.where(j % 4 == 1, qr - np.uint64(1), np.where(j % 4 == 2, (qr - a) % qr, (qr - np.uint64(1) - a + qr) % qr)))
    return out


class Uniform:
    """family U of tests/keyswitch_craft.py restated for L rows: every source residue is the CONSTANT polynomial q_i - 1, so its transform
    modulo q_r holds a = (q_i - 1) mod q_r in every slot, whatever the slot order (a Galois automorphism leaves a constant alone); the key
    holds, per slot, residues e = tau a^-1 mod q_r for which mulvv_pm(a, e) = tau + q_r: each of the L lazy products of every slot of the
    pseudo-Mersenne accumulation is above q_r.  pm=False: the same construction with canonical products (the general path's control)."""

    def __init__(self, q, n, pm=True):
        import keyswitch_craft as kc
        from test_pm_arithmetic_model import Pm
        self.q, self.n, self.k, self.L, self.pm = list(q), n, len(q), len(q) - 1, pm
        self.a = [[(q[i] - 1) % q[r] for r in range(self.k)] for i in range(self.L)]
        assert all(v for row in self.a for v in row)
        self.res = {}
        for i in range(self.L):
            for r in range(self.k):
                a = self.a[i][r]
                if pm:
                    found, _ = kc.qualifying(a, Pm(q[r]), want=8)
                    assert found, "no key residue with a lazy product above q"
                else:
                    inv = pow(a, -1, q[r])
                    found = [t * inv % q[r] for t in range(1, 9)]
                self.res[(i, r)] = found

    def source(self):
        d = np.zeros((self.L, self.n), dtype=np.uint64)
        for i in range(self.L):
            d[i, 0] = self.q[i] - 1
        return d

    def key(self):
        """[L][2][k][n] in NTT form, valid in ANY slot order only through its use: slot s of (i, pp, r) holds residue (s + 5 pp + i) mod 8 --
        the oracle and the library index slots differently, so the key is handed to each side in COEFFICIENT form (key_coeff)"""
        key = np.zeros((self.L, 2, self.k, self.n), dtype=np.uint64)
        slots = np.arange(self.n)
        for i in range(self.L):
            for r in range(self.k):
                e = np.array(self.res[(i, r)], dtype=np.uint64)
                for pp in range(2):
                    key[i, pp, r] = e[(slots + 5 * pp + i) % len(e)]
        return key

    def key_coeff(self, orc):
        """the key whose ORACLE NTT form is key(): both sides then multiply the same residue polynomials (each slot of either order holds one
        of the eight crafted residues, as a set)"""
        key = self.key()
        out = np.zeros_like(key)
        for idx in np.ndindex(key.shape[:2]):
            for r in range(self.k):
                out[idx + (r,)] = orc.ntt_inv(key[idx + (r,)], r)
        return out
