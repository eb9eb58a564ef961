"""The key switch (csrc/behz.hip k_relin_*, csrc/galois.hip k_galois_*) restated for ONE NTT slot in Python integers, the host's
choices around it (digit count, the 20-term gate, the pass grouping of fhe_relinearize_n), and operands crafted with both.  No GPU
imports, no library; tests/test_keyswitch_craft_cpu.py proves in the model that every target is reached,
tests/test_gpu_keyswitch_extremes.py runs the operands through the kernels.

One slot of the key switch, for source prime i, digit d, target prime ii, output polynomial pp:
  x   = (c_i >> (dbc d)) & (2^dbc - 1)                     the digit of the source residue
  x'  = fold_pm(x) where dbc >= bits(q_ii)                  the kernels' `wide` test; x' < 2^(b+1) enters the forward transform
  a   = x mod q_ii, canonical                               what canon_pm leaves in the digit array (NTT form)
  pseudo-Mersenne path:  S = sum_(power, i, d) mulvv_pm(a, e)   plain 64-bit additions of lazy products, then ONE fold_pm(S)
  general path:          S = sum a e mod q_ii                   canonical products, addmod
  the inverse transform of S, canonical, is added to c0 / c1 with addmod

Two families of operands:
  U  every source polynomial is a constant (coefficient 0 only), so every digit polynomial is a constant and its transform holds
     a = digit mod q_ii in EVERY slot, whatever the slot order; a Galois automorphism leaves it alone.  The key is then free per slot:
     it holds residues e = t a^-1 mod q_ii, t small, for which mulvv_pm(a, e) = t + q_ii -- a lazy product above q_ii in every term of
     every sum --, or q_ii - 1 everywhere, or 0 in polynomial 1.
  D  real keys; every coefficient of the source carries a chosen digit pattern, and whole polynomials carry the digit maximum.
"""
import random

import numpy as np

from galois_oracle import Q3, Q4
from test_pm_arithmetic_model import Pm, fold_pm, is_prime, mulvv_pm, u64

MAX_TERMS = 20                    # relin_pm_ok: k x digits x powers
CONTROL_TERMS = 24                # the general-path control runs of family U: sums this long are canonical there anyway
T_PLAIN = 1 << 14
SEARCH_T = 2000


def primes_58(n, count=2):
    """the largest `count` 58-bit primes = 1 (mod 2n): pseudo-Mersenne class B"""
    out, m = [], (1 << 58) + 1
    while len(out) < count:
        m -= 2 * n
        if is_prime(m):
            out.append(m)
    return out


# name -> (n, q, switches, pseudo-Mersenne class the key switch must run on: fhe_arith_path & 3)
BASES = {
    "A": (1024, Q4, {}, 1),                                            # the P8192 primes, 55/55/54/54 bits
    "B": (1024, primes_58(1024), {}, 2),
    "A-nopm": (1024, Q4, {"FHE_NTT_NOPM": 1}, 0),                      # general path, Shoup transforms
    "P4096-n1024": (1024, Q3, {}, 0),                                  # general path
    "P4096": (4096, Q3, {}, 0),                                        # general path, exact-FP64 transforms
}
SIZES_N = {"A": (1024, 2048, 4096, 8192), "B": (1024, 8192)}          # every transform size the key switch instantiates


def base_at(name, n):
    """(q, switches, class) of base `name` at another n: class B needs primes = 1 (mod 2n)"""
    _, q, sw, cls = BASES[name]
    return (primes_58(n) if name == "B" else q), sw, cls


# ---- the host's choices -------------------------------------------------------------------------------------------------------------
def digits(q, dbc):
    """fhe_evk_digits: the digit count comes from the widest prime"""
    return -(-max(p.bit_length() for p in q) // dbc)


def gate(k, nd, npow=1):
    """relin_pm_ok, the part that depends on the shape"""
    return k * nd * npow <= MAX_TERMS


def passes(size, k, nd, pm=True, steps=False):
    """fhe_relinearize_n: the polynomials [lo, hi] of every pass, in order.  As few passes as the gate allows, from the top, gmax
    polynomials at a time; one polynomial per pass on the general path, under FHE_RELIN_STEPS and where not even two powers fit"""
    gmax = size - 2
    while gmax > 1 and not gate(k, nd, gmax):
        gmax -= 1
    if not pm or steps or size <= 3 or gmax <= 1:
        return [(p, p) for p in range(size - 1, 1, -1)]
    out, hi = [], size - 1
    while hi >= 2:
        g = min(hi - 1, gmax)
        lo = hi - g + 1
        out.append((lo, hi))
        hi = lo - 1
    return out


def dbc_rule(q):
    """the decomposition bit counts a base is tested at, by rule"""
    k = len(q)
    widths = sorted({p.bit_length() for p in q})
    out = {60, 1, 31, 32, 33}
    for b in widths:
        out |= {b - 1, b, min(b + 1, 60)}                               # the `wide` boundary dbc >= b of every prime width
    first = min(d for d in range(1, 61) if gate(k, digits(q, d)))
    out |= {first, first - 1} if first > 1 else {first}                 # the longest lazy sum, and the first dbc on the general path
    out |= {d for d in range(1, 61) if -(-widths[-1] // d) != -(-widths[0] // d)}      # the narrowest prime has fewer digits than the widest
    return sorted(out)


def twenty_term_dbc(q):
    return min(d for d in range(1, 61) if gate(len(q), digits(q, d)))


def control_dbc(q):
    return min(d for d in range(1, 61) if len(q) * digits(q, d) <= CONTROL_TERMS)


# ---- one slot -----------------------------------------------------------------------------------------------------------------------
def digit_of(v, dbc, d):
    return (v >> (dbc * d)) & ((1 << dbc) - 1)


def stored_digit(v, dbc, d, m, pm):
    """the canonical digit residue the accumulation reads: k_relin_fwd_pm / k_galois_fwd_pm (pm) or k_relin_digits / k_galois_digits"""
    x = u64(digit_of(v, dbc, d))
    if not pm:
        return x % m.q
    if dbc >= m.sh + 32:                                   # `wide`: the digit may reach q_ii
        x = fold_pm(x, m)
    assert x < (1 << (m.b + 1))                            # what the forward transform and mulvv_pm take
    y = fold_pm(x, m)                                      # canon_pm: fold, one conditional subtraction
    y = y - m.q if y >= m.q else y
    assert y < m.q and y == digit_of(v, dbc, d) % m.q
    return y


_products = {}


def lazy_product(a, e, m):
    key = (a, e, m.q)
    if key not in _products:
        _products[key] = mulvv_pm(a, e, m)
    return _products[key]


def slot_sum(terms, m, pm):
    """terms: [(a, e)] of one slot.  Returns (the 64-bit sum before the fold, the folded value, the canonical value); on the general path all
    three are the canonical sum"""
    if not pm:
        s = 0
        for a, e in terms:
            s = (s + a * e % m.q) % m.q
        return s, s, s
    s = 0
    for a, e in terms:
        s = u64(s + lazy_product(a, e, m))
    f = fold_pm(s, m)
    assert f - m.q < m.q                                   # fold_pm leaves the value mod q or that plus q: at most one q to take off
    return s, f, f % m.q


def qualifying(a, m, want=None, tmax=SEARCH_T):
    """key residues e = t a^-1 mod q, t = 1 .. tmax - 1, whose lazy product with a is at or above q (a e = t mod q: the product is then
    t + q), and the (result, e) with the largest result seen.  want: stop after that many"""
    inv = pow(a, -1, m.q)
    out, best = [], (0, 0)
    for t in range(1, tmax):
        e = t * inv % m.q
        r = lazy_product(a, e, m)
        best = max(best, (r, e))
        if r >= m.q:
            out.append(e)
            if want and len(out) == want:
                break
    return out, best


# ---- family U -----------------------------------------------------------------------------------------------------------------------
def max_source(qi, dbc):
    """the source constant: q_i - 1 when one digit holds it; else every digit all ones except the top one, the largest that keeps the
    residue below q_i (should that top digit be 0, q_i - 1 itself: every digit has to be non-zero)"""
    b = qi.bit_length()
    if dbc >= b:
        return qi - 1
    s = dbc * (-(-b // dbc) - 1)
    ones, topmax = (1 << s) - 1, (qi - 1) >> s
    for top in (topmax, topmax - 1):
        if top >= 1 and ((top << s) | ones) < qi:
            return (top << s) | ones
    return qi - 1


class Uniform:
    """family U for base q at n, dbc and `npow` powers (a ciphertext of npow + 2 polynomials)"""
    KINDS = ("crafted", "qm1", "zero1")

    def __init__(self, q, n, dbc, npow, pm):
        self.q, self.n, self.dbc, self.npow, self.pm = list(q), n, dbc, npow, bool(pm)
        self.k, self.nd = len(q), digits(q, dbc)
        self.mods = [Pm(p) for p in q]
        self.src = [max_source(p, dbc) for p in q]
        assert all(v < p for v, p in zip(self.src, q))
        # reachable digits that are zero all the same (none on the pseudo-Mersenne cases the tests run: asserted there)
        self.zero_digits = [(i, d) for i, v in enumerate(self.src) for d in range(-(-q[i].bit_length() // dbc)) if not digit_of(v, dbc, d)]
        # a[i][d][ii]; 0 only above the top digit of a prime narrower than the widest
        self.a = [[[stored_digit(self.src[i], dbc, d, self.mods[ii], self.pm) for ii in range(self.k)] for d in range(self.nd)] for i in range(self.k)]
        self.unreached = []                                # (i, d, ii, a) whose lazy product cannot reach q_ii; empty at dbc >= bits
        self.best = {}                                     # (i, ii) -> (largest lazy product the search found, a, e)
        self._keys = {}

    def _residues(self, i, d, ii):
        """the key residues slot s of (i, d, ii) cycles through"""
        a, m = self.a[i][d][ii], self.mods[ii]
        if a == 0:
            return [m.q - 1]
        if not self.pm:                                    # the control: the same construction, canonical products
            inv = pow(a, -1, m.q)
            return [t * inv % m.q for t in range(1, 9)]
        found, best = qualifying(a, m, want=8)
        self.best[(i, ii)] = max(self.best.get((i, ii), (0, 0, 0)), best[:1] + (a,) + best[1:])
        if not found:                                      # a digit of a few bits (the top digit below dbc = bits): a e < q for every e it
            self.unreached.append((i, d, ii, a))           # could reach q with; the largest product it has instead
            return [m.q - 1]
        return found

    def key(self, kind="crafted"):
        """[npow][k][nd][2][k][n], the oracle's NTT form (any slot order: a is the same in every slot)"""
        if kind not in self._keys:
            key = np.zeros((self.npow, self.k, self.nd, 2, self.k, self.n), dtype=np.uint64)
            slots = np.arange(self.n)
            for i in range(self.k):
                for d in range(self.nd):
                    for ii in range(self.k):
                        if kind == "qm1":
                            key[:, i, d, :, ii, :] = self.q[ii] - 1
                            continue
                        r = np.array(self._residues(i, d, ii), dtype=np.uint64)
                        for pw in range(self.npow):
                            for pp in range(2):
                                key[pw, i, d, pp, ii] = r[(slots + 3 * pw + 5 * pp + i + d) % len(r)]
            if kind == "zero1":
                key[:, :, :, 1] = 0
            self._keys[kind] = key
        return self._keys[kind]

    def ct(self, size=None, c01=None):
        """[size][k][n]: c0 / c1 as given (zero otherwise), every polynomial from 2 on the constant"""
        size = self.npow + 2 if size is None else size
        ct = np.zeros((size, self.k, self.n), dtype=np.uint64)
        if c01 is not None:
            ct[:2] = c01
        for i in range(self.k):
            ct[2:, i, 0] = self.src[i]
        return ct

    def slots(self, key, lo=2, hi=None):
        """the model: (sum, folded, canonical) arrays [2][k][n] (Python integers) of ONE pass over the polynomials lo .. hi"""
        hi = self.npow + 1 if hi is None else hi
        out = [np.zeros((2, self.k, self.n), dtype=object) for _ in range(3)]
        for pp in range(2):
            for ii in range(self.k):
                m, seen = self.mods[ii], {}
                av = [self.a[i][d][ii] for p in range(lo, hi + 1) for i in range(self.k) for d in range(self.nd)]
                ev = key[lo - 2:hi - 1, :, :, pp, ii, :].reshape(len(av), self.n).T.tolist()      # [slot][term]
                for s in range(self.n):
                    es = tuple(ev[s])
                    if es not in seen:                     # the key cycles through a few residues: equal slots are computed once
                        seen[es] = slot_sum(list(zip(av, es)), m, self.pm)
                    for o, v in zip(out, seen[es]):
                        o[pp, ii, s] = v
        return out

    def finish(self, orc, canon, c01):
        """a pass's canonical slot values through the oracle's own inverse transform and addition"""
        out = np.array(c01, dtype=np.uint64).copy()
        for pp in range(2):
            for ii in range(self.k):
                acc = orc.ntt_inv(np.array([int(v) for v in canon[pp, ii]], dtype=np.uint64), ii)
                out[pp, ii] = (out[pp, ii] + acc) % np.uint64(self.q[ii])           # both below 2^61
        return out

    def model_relinearize(self, orc, key, c01, steps=False):
        """the whole call: every pass of fhe_relinearize_n (one pass for npow = 1)"""
        out = np.array(c01, dtype=np.uint64)
        for lo, hi in passes(self.npow + 2, self.k, self.nd, self.pm, steps):
            out = self.finish(orc, self.slots(key, lo, hi)[2], out)
        return out


def final_addends(acc, q):
    """c0 / c1 [2][k][n] for the final addmod, per coefficient in turn: 0, q - 1, the value that makes the sum exactly q (result 0) and the
    one that makes it q - 1; acc: what the key switch adds (an oracle run with c0 = c1 = 0)"""
    acc = np.asarray(acc, dtype=np.uint64)
    out = np.zeros_like(acc)
    j = np.arange(acc.shape[-1])
    for ii, qi in enumerate(q):
        qi = np.uint64(qi)
        a = acc[:, ii]
        out[:, ii] = np.where(j % 4 == 0, np.uint64(0), np.where(j % 4 == 1, qi - np.uint64(1), np.where(j % 4 == 2, (qi - a) % qi, (qi - np.uint64(1) - a + qi) % qi)))
    return out


# ---- family D -----------------------------------------------------------------------------------------------------------------------
def digit_targets(q, i, dbc):
    """[(digit position, value)] for source prime i: 0, 1, 2^dbc - 2, 2^dbc - 1 at every position; q_ii - 1, q_ii, q_ii + 1 where the digit can
    reach them; at the top position its own maximum (and one below) and one above what each narrower prime can hold there.  Values a
    position cannot hold are left out; a position above the prime's own top digit is always 0 and gets no target"""
    qi = q[i]
    ndi = -(-qi.bit_length() // dbc)
    full = (1 << dbc) - 1
    out = []
    for d in range(ndi):
        cap = full if d < ndi - 1 else (qi - 1) >> (dbc * d)
        want = {0, 1, full - 1, full}
        for qq in q:
            if dbc >= qq.bit_length():
                want |= {qq - 1, qq, qq + 1}
        if d == ndi - 1:
            want |= {cap, cap - 1}
            want |= {((qq - 1) >> (dbc * d)) + 1 for qq in q if qq.bit_length() < qi.bit_length()}
        out += [(d, v) for v in sorted(want) if 0 <= v <= cap]
    return out


def digit_poly(q, n, dbc, seed=1):
    """[k][n]: coefficient j of prime i carries target j mod len(targets_i); the other digits are random.  Coefficient n - 1 is 0 in every
    prime (the value whose negation is 0).  Returns (polynomial, {i: targets})"""
    rng = random.Random(seed * 1000 + dbc)
    poly = np.zeros((len(q), n), dtype=np.uint64)
    targets = {}
    for i, qi in enumerate(q):
        tg = digit_targets(q, i, dbc)
        assert len(tg) < n
        targets[i] = tg
        ndi = -(-qi.bit_length() // dbc)
        s_top = dbc * (ndi - 1)
        topmax, low_qm1 = (qi - 1) >> s_top, (qi - 1) & ((1 << s_top) - 1)
        for j in range(n - 1):
            d, v = tg[j % len(tg)]
            if d == ndi - 1:
                low = rng.randrange(low_qm1 + 1) if v == topmax else rng.randrange(1 << s_top)
                x = (v << s_top) | low
            else:
                x = (rng.randrange(topmax) << s_top) | rng.randrange(1 << s_top)
                x = (x & ~(((1 << dbc) - 1) << (dbc * d))) | (v << (dbc * d))
            assert x < qi and digit_of(x, dbc, d) == v
            poly[i, j] = x
    return poly, targets


def whole_polys(q, n, dbc):
    """[2 + log2 n][k][n]: every coefficient at the digit maximum (max_source: every digit polynomial at ITS largest magnitude), the maximum at
    even and 0 at odd indices, and the maximum where index bit b is set, one polynomial per bit"""
    top = np.array([max_source(p, dbc) for p in q], dtype=np.uint64)[:, None]
    j = np.arange(n)[None, :]
    zero = np.uint64(0)
    out = [np.broadcast_to(top, (len(q), n)).copy(), np.where(j % 2 == 0, top, zero)]
    out += [np.where((j >> b) & 1 == 1, top, zero) for b in range(n.bit_length() - 1)]
    return np.stack(out).astype(np.uint64)


def digit_sources(q, n, dbc):
    """the source polynomials of family D [1 + 2 + log2 n][k][n] and the targets of the first"""
    poly, targets = digit_poly(q, n, dbc)
    return np.concatenate([poly[None], whole_polys(q, n, dbc)]), targets


def negated_positions(n, g):
    """stored index s of a polynomial -> whether sigma_g negates it (s g mod 2n >= n)"""
    return (np.arange(n, dtype=np.int64) * g % (2 * n)) >= n


def direct_form(target, g, q):
    """the stored polynomial [.., k, n] whose value v at every position sigma_g negates is q_i - pattern (0 for the pattern 0), so that the
    kernel's negation modulo the SOURCE prime, before the digit is taken, produces the pattern; elsewhere the pattern itself"""
    target = np.asarray(target, dtype=np.uint64)
    neg = negated_positions(target.shape[-1], g)
    out = target.copy()
    for i, qi in enumerate(q):
        v = target[..., i, :]
        out[..., i, :] = np.where(neg & (v != 0), np.uint64(qi) - v, v)
    return out
