"""Specification of modulus switching (include/fhe_hip.h: fhe_mod_switch) in three forms, none of which calls the library:
  * switch_big: the definition on big integers -- compose c in [0, q) by CRT, c' = floor((c + floor(p / 2)) / p) mod (q / p) per dropped
    prime p, last prime first, decompose;
  * switch_residues: the residue form c'_i = (c_i + (h mod q_i) - (r mod q_i)) p^-1 mod q_i with r = (c_m + h) mod p, vectorised over
    numpy object arrays (the GPU tests' reference: every level of one input comes from one walk down);
  * switch_model: the residue form as csrc/modswitch.hip computes it, one coefficient at a time, with every 64-bit register passed through
    u64() -- the unsigned addend A = (h mod q_i) + M, M the smallest multiple of q_i that is >= p, the Shoup product of x = c_i + A - r with
    p^-1 and the conditional subtractions -- and, on request, one of the WRONG variants the crafted operands are there to catch.
tests/test_modswitch_cpu.py checks the three against each other; craft() builds operands backwards from prescribed remainders and results."""
from functools import reduce

import numpy as np

import galois_oracle as go

M64 = (1 << 64) - 1
Q3, Q4 = go.Q3, go.Q4                                                 # 36/36/37 bits (the dropped prime is the larger one); 55/55/54/54 bits
S16K = [0x7FFFFFFF380001, 0x7FFFFFFEF00001, 0x7FFFFFFEAC0001, 0x7FFFFFFE700001, 0x7FFFFFFE600001, 0x7FFFFFFE4C0001, 0x3FFFFFFF000001, 0x3FFFFFFEF40001]
R_TARGETS = ("0", "1", "h-1", "h", "h+1", "p-2", "p-1")
C_TARGETS = ("0", "1", "q-2", "q-1")
VARIANTS = ("gt_final", "gt_r", "raw_r")


def _is_prime(m):
    if m < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if m % p == 0:
            return m == p
    d, s = m - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):          # a proof below 3.3e24
        x = pow(a, d, m)
        if x in (1, m - 1):
            continue
        for _ in range(s - 1):
            x = x * x % m
            if x == m - 1:
                break
        else:
            return False
    return True


def primes_below(bits, n, count):
    """the largest `count` primes below 2^bits that are 1 (mod 2n)"""
    out, m = [], (1 << bits) + 1
    while len(out) < count:
        m -= 2 * n
        if _is_prime(m):
            out.append(m)
    return out


def bases(n=1024):
    """name -> primes: the six bases of the issue"""
    p61 = primes_below(61, n, 1)[0]
    return {"Q3": list(Q3), "Q4": list(Q4), "Q58": primes_below(58, n, 2), "Q61": [p61, Q4[0]], "Q61R": [Q4[0], p61], "S16K": list(S16K)}


def u64(v):
    assert 0 <= v <= M64, "64-bit register overflow"
    return v


def prod(q):
    return reduce(lambda a, b: a * b, q, 1)


def compose(res, q):
    Q = prod(q)
    return sum(int(r) * (Q // qi) * pow(Q // qi, -1, qi) for r, qi in zip(res, q)) % Q


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
def drop_big(c, q):
    """one drop of the last prime of the base q on the canonical representative"""
    p = q[-1]
    return ((c + p // 2) // p) % prod(q[:-1])


def switch_big(res, q, k_out):
    """residues [k] of one coefficient -> residues [k_out] after k - k_out iterated drops"""
    q = list(q)
    c = compose(res, q)
    while len(q) > k_out:
        c = drop_big(c, q)
        q.pop()
    return [c % qi for qi in q]


# ---- the residue form, vectorised ---------------------------------------------------------------------------------------------------------
def switch_residues_levels(x, q):
    """x: uint64 [..., k, n] -> {k_out: uint64 [..., k_out, n]} for every k_out in 1 .. k - 1 (one walk down: the iteration is the definition)"""
    cur = [np.asarray(x[..., i, :]).astype(object) for i in range(len(q))]
    out = {}
    for m in range(len(q) - 1, 0, -1):
        p, h = q[m], q[m] // 2
        r = (cur[m] + h) % p
        cur = [(cur[i] + h % q[i] - r % q[i]) % q[i] * pow(p, -1, q[i]) % q[i] for i in range(m)]
        out[m] = np.stack([c.astype(np.uint64) for c in cur], axis=-2)
    return out


# ---- the residue form in 64-bit registers, as the kernel has it -----------------------------------------------------------------------------
def _csub(x, q, strict=False):
    return x - q if (x > q if strict else x >= q) else x


def _mul_shoup(x, w, wp, q, strict=False):
    """csrc/modarith.h mul_shoup: any 64-bit x; the lazy product is x w - floor(x wp / 2^64) q modulo 2^64, below 2 q"""
    lazy = (u64(x) * w - ((x * wp) >> 64) * q) & M64
    assert lazy < 2 * q
    return _csub(lazy, q, strict)


_PAIR = {}


def _pair(p, qi):
    """what the host precomputes per (dropped p, kept q_i): p^-1 mod q_i, its Shoup companion, h mod q_i, the unsigned addend"""
    if (p, qi) not in _PAIR:
        inv = pow(p, -1, qi)
        _PAIR[(p, qi)] = (inv, (inv << 64) // qi, (p >> 1) % qi, u64((p >> 1) % qi + (p + qi - 1) // qi * qi))
    return _PAIR[(p, qi)]


def switch_model(res, q, k_out, variant=None, trace=None):
    """one coefficient through the kernel's arithmetic.  variant: None, or
         "gt_final": `>` for `>=` in the last conditional subtraction of a product (a result of exactly q_i stays q_i),
         "gt_r":     `>` for `>=` in the reduction of c_m + h (a remainder of exactly 0 stays p),
         "raw_r":    r subtracted as if it were below q_i: x = c_i + (h mod q_i) + q_i - r in a 64-bit register (wraps when r is larger).
    trace, when a list, receives the rounded remainder r of every drop, last prime first."""
    assert variant is None or variant in VARIANTS
    a = [int(v) for v in res]
    for m in range(len(q) - 1, k_out - 1, -1):
        p, h = q[m], q[m] >> 1
        r = _csub(u64(a[m] + h), p, strict=variant == "gt_r")
        if trace is not None:
            trace.append(r)
        for i in range(m):
            qi = q[i]
            inv, invp, hm, add = _pair(p, qi)
            if variant == "raw_r":
                x = (a[i] + hm + qi - r) & M64
            else:
                x = u64(u64(a[i] + add) - r)
            a[i] = _mul_shoup(x, inv, invp, qi, strict=variant == "gt_final")
    return a[:k_out]


# ---- crafted operands ----------------------------------------------------------------------------------------------------------------------
def _r_value(name, p):
    h = p // 2
    return {"0": 0, "1": 1, "h-1": h - 1, "h": h, "h+1": h + 1, "p-2": p - 2, "p-1": p - 1}[name]


def _c_value(name, qi):
    return {"0": 0, "1": 1, "q-2": qi - 2, "q-1": qi - 1}[name]


def build_backwards(final, rs, q, k_out):
    """final: the k_out residues of the result; rs: {m: r_m} the rounded remainder of the drop of q_m, m = k_out .. k - 1.  Returns the k
    residues of the operand: c^(j+1) = c^(j) p_j + (r_j - h_j) mod q^(j+1) going up, so that floor((c^(j+1) + h_j) / p_j) = c^(j) -- also
    when r_j < h_j at c^(j) = 0, where c^(j+1) wraps to the top of [0, q^(j+1)) and c + h passes q."""
    c = compose(final, q[:k_out])
    for j in range(k_out, len(q)):
        c = (c * q[j] + rs[j] - q[j] // 2) % prod(q[:j + 1])
    return [c % qi for qi in q]


def craft(q, k_out, seed=0):
    """[(residues [k], what it prescribes)]: every r target at every drop under every final target (the other drops' remainders random),
    and, built forwards, c = 0, 1, q - 1 and c on both sides of q - h, where c + h wraps"""
    rng = np.random.default_rng(seed)
    k = len(q)
    rnd = lambda m: int(rng.integers(0, q[m]))
    out = []
    for m in range(k_out, k):
        for rt in R_TARGETS:
            for ct in C_TARGETS:
                rs = {j: _r_value(rt, q[j]) if j == m else rnd(j) for j in range(k_out, k)}
                final = [_c_value(ct, q[i]) for i in range(k_out)]
                out.append((build_backwards(final, rs, q, k_out), ("r", m, rt, ct)))
    Q, h = prod(q), q[-1] // 2
    for name, c in (("c=0", 0), ("c=1", 1), ("c=q-1", Q - 1), ("c=q-2", Q - 2), ("c=q/2", Q // 2), ("c=h", h), ("c=h+1", h + 1), ("c=q-h-1", Q - h - 1), ("c=q-h", Q - h)):
        out.append(([c % qi for qi in q], (name,)))
    return out


def crafted_tile(q, k_out, n, seed=0):
    """uint64 [k, n]: the crafted coefficient list of (q, k_out), tiled across a polynomial"""
    ops = [r for r, _ in craft(q, k_out, seed)]
    return np.array([[ops[c % len(ops)][i] for c in range(n)] for i in range(len(q))], dtype=np.uint64)


# ---- a toy BFV in Python integers (noise bound) ---------------------------------------------------------------------------------------------
def negacyclic_mul(a, b, mod):
    n = len(a)
    out = [0] * n
    for i, x in enumerate(a):
        if not x:
            continue
        for j, y in enumerate(b):
            if i + j < n:
                out[i + j] += x * y
            else:
                out[i + j - n] -= x * y
    return [v % mod for v in out]
