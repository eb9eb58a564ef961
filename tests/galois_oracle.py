"""Specification of the Galois rotations (include/fhe_hip.h "batched plaintext slots and Galois rotations") on the UNCHANGED CPU oracle:
sigma_g in numpy, Galois keys built from a secret key in Python integers, apply_galois as Oracle.relinearize of [sigma(c0), 0, sigma(c1)],
and a slot encoder in Python integers.  Nothing here calls the library: its encoder, its index map and its key generator are checked
against these restatements."""
import numpy as np

Q3 = [0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001]                                              # the P4096 primes (general / FP64-transform path)
Q4 = [0x7FFFFFFF380001, 0x7FFFFFFEF00001, 0x3FFFFFFF000001, 0x3FFFFFFEF40001]              # the P8192 primes (pseudo-Mersenne class 1)
T_BATCH = 65537


# ---- the automorphism -------------------------------------------------------------------------------------------------------------
def sigma(a, g, q):
    """x^i -> x^(i g mod 2n), x^n = -1, on residues [..., k, n]: coefficient i goes to e = i g mod 2n if e < n, else to e - n negated
    modulo q_i (the negation of 0 is 0)"""
    a = np.asarray(a, dtype=np.uint64)
    n = a.shape[-1]
    assert g % 2 == 1 and 1 < g < 2 * n
    e = np.arange(n, dtype=np.int64) * g % (2 * n)
    out = np.zeros_like(a)
    for r, qr in enumerate(q):
        v = a[..., r, :]
        out[..., r, e % n] = np.where(e >= n, np.where(v == 0, np.uint64(0), np.uint64(qr) - v), v)
    return out


def elements(n):
    """the test cases' Galois elements and the slot permutation each must produce: (g, rows rotated left by, rows swapped)"""
    return [(3, 1, False), (pow(3, -1, 2 * n), -1, False), (2 * n - 1, 0, True), (pow(3, n // 8, 2 * n), n // 8, False)]


def permute_slots(slots, left, swap):
    """flat slots [.., n] (row 0 then row 1): both rows rotated left by `left`, then swapped"""
    s = np.asarray(slots)
    n = s.shape[-1]
    rows = np.roll(s.reshape(s.shape[:-1] + (2, n // 2)), -left, axis=-1)
    if swap:
        rows = rows[..., ::-1, :]
    return rows.reshape(s.shape)


# ---- Galois keys in the oracle's layout ---------------------------------------------------------------------------------------------
def _obj(a):
    return np.array([int(x) for x in a], dtype=object)


def galois_key(orc, sk, g, dbc, seed=1):
    """[k][digits][2][k][n] in the oracle's NTT form, the layout and digit rule of its evaluation keys, for the target sigma_g(s):
    entry (i, d) = (-(a s + e) + 2^(dbc d) sigma_g(s) on component i only, a).  a uniform, e uniform in [-3, 3] (a test key)."""
    rng = np.random.default_rng(seed)
    k, n, q = orc.k, orc.n, orc.q
    nd = (max(x.bit_length() for x in q) + dbc - 1) // dbc
    S = [_obj(orc.ntt_fwd(sk[r], r)) for r in range(k)]
    target = sigma(sk, g, q)
    T = [_obj(orc.ntt_fwd(target[r], r)) for r in range(k)]
    key = np.zeros((k, nd, 2, k, n), dtype=np.uint64)
    for i in range(k):
        for d in range(nd):
            e = rng.integers(-3, 4, size=n)
            for r in range(k):
                qr = q[r]
                A = _obj(rng.integers(0, qr, size=n, dtype=np.uint64))
                E = _obj(orc.ntt_fwd(np.array([int(x) % qr for x in e], dtype=np.uint64), r))
                k0 = (-(A * S[r] + E)) % qr
                if r == i:
                    k0 = (k0 + pow(2, dbc * d, qr) * T[r]) % qr
                key[i, d, 0, r] = np.array(list(k0), dtype=np.uint64)
                key[i, d, 1, r] = np.array(list(A), dtype=np.uint64)
    return key


def apply_galois(orc, ct, g, key, dbc):
    """the specification: relinearize-step([sigma_g(c0), 0, sigma_g(c1)]) with the key for sigma_g(s)"""
    ct = np.asarray(ct, dtype=np.uint64)
    assert ct.shape == (2, orc.k, orc.n)
    s = sigma(ct, g, orc.q)
    three = np.stack([s[0], np.zeros_like(s[0]), s[1]])
    return orc.relinearize(np.ascontiguousarray(three), np.ascontiguousarray(key), dbc)


def key_to_oracle(orc, key_coeff):
    """a key in coefficient form (the library's, taken back with ntt_inverse) in the oracle's NTT form: each side keeps its own slot order"""
    out = np.zeros_like(key_coeff)
    for idx in np.ndindex(key_coeff.shape[:3]):
        for r in range(orc.k):
            out[idx + (r,)] = orc.ntt_fwd(key_coeff[idx + (r,)], r)
    return out


# ---- slots, in Python integers ------------------------------------------------------------------------------------------------------
def is_prime(t):
    if t < 2:
        return False
    i = 2
    while i * i <= t:
        if t % i == 0:
            return False
        i += 1
    return True


def slot_root(n, t):
    """the smallest primitive 2n-th root of unity modulo the prime t = 1 (mod 2n)"""
    assert is_prime(t) and (t - 1) % (2 * n) == 0
    for z in range(2, t):
        if pow(z, n, t) == t - 1:          # order divides 2n and not n: for a power of two 2n, the order is 2n
            return z
    raise ValueError("no root")


def slot_exponents(n):
    """exponent e of flat slot index: 3^j mod 2n for row 0, 2n - 3^j for row 1"""
    row0 = [pow(3, j, 2 * n) for j in range(n // 2)]
    return row0 + [2 * n - e for e in row0]


def _eval_odd_powers(m, z, t):
    """{e: m(z^e)} for every odd e below 2 len(m), z a primitive 2 len(m)-th root: m(x) = even(x^2) + x odd(x^2), and the squares of the
    odd powers of z are the odd powers of z^2"""
    ln = len(m)
    if ln == 1:
        return {1: m[0] % t}
    ev, od = _eval_odd_powers(m[0::2], z * z % t, t), _eval_odd_powers(m[1::2], z * z % t, t)
    out, p, zz = {}, z, z * z % t
    for e in range(1, 2 * ln, 2):
        out[e] = (ev[e % ln] + p * od[e % ln]) % t
        p = p * zz % t
    return out


def decode_slots(plain, n, t):
    vals = _eval_odd_powers([int(x) for x in plain], slot_root(n, t), t)
    return np.array([vals[e] for e in slot_exponents(n)], dtype=np.uint64)


def _eval_all_powers(v, w, t):
    """[V(w^c) for c in 0 .. len(v) - 1], w a primitive len(v)-th root of unity"""
    ln = len(v)
    if ln == 1:
        return [v[0] % t]
    ev, od = _eval_all_powers(v[0::2], w * w % t, t), _eval_all_powers(v[1::2], w * w % t, t)
    out, p = [0] * ln, 1
    for c in range(ln):
        out[c] = (ev[c % (ln // 2)] + p * od[c % (ln // 2)]) % t
        p = p * w % t
    return out


def encode_slots(slots, n, t):
    """the plaintext whose slots are `slots`: m_c = n^-1 zeta^-c V(zeta^-2c) with V(y) = sum_i v_(2i+1) y^i, v_e the value at zeta^e"""
    z = slot_root(n, t)
    v = [0] * n
    for val, e in zip(slots, slot_exponents(n)):
        assert int(val) < t
        v[(e - 1) // 2] = int(val)
    iz = pow(z, -1, t)
    big = _eval_all_powers(v, iz * iz % t, t)
    ninv = pow(n, -1, t)
    return np.array([big[c] * ninv * pow(iz, c, t) % t for c in range(n)], dtype=np.uint64)
