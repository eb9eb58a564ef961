"""The transform kernels (csrc/ntt_core.h; k_ntt_fwd*, k_ntt_inv*, k_mulplain* of csrc/fhe_hip.hip; k_poly_f64 of csrc/dct_fused.hip)
restated in Python integers as ONE butterfly network over the natural coefficient index, and operands crafted so that chosen OUTPUTS are
0, 1, 2, floor(q/2), floor(q/2) + 1, q - 2, q - 1.  No GPU imports, no library; tests/test_ntt_craft_cpu.py proves in the model that the
targets are reached in their non-canonical (lazy) form, tests/test_gpu_ntt_extremes.py runs the same operands through the kernels.

What is modelled: the VALUE of every register.  Which thread and register holds index j changes no value, so the layout (register passes,
LDS transposes, slot order) is not modelled -- except that the inverse passes track their ranges per REGISTER index r = (j >> LO) & 15 of
the pass, which the plans below restate.  Every intermediate a kernel keeps in a 64-bit register goes through u64(), so a wrap raises; the
multiply-add chain of mul_shoup_lazy4 is arithmetic modulo 2^64 by design and is checked as a whole (result = acc + x w - qhat q as
integers, qhat in [exact - 3, exact], product below 4 q).

Models (each returns a Run: lazy value of every output before canonicalisation, canonical output, per stage (label, static bound, largest
operand) in sixteenths of q) and the bound each asserts:
  pm_forward / pm_inverse / pm_multiply_plain   classes A and B; pm_fwd_bound's fold schedule, pm_inv_plan; mul_pm operands <= LIM q,
                                                mulvv_pm operands < 2^(b+1), canon_pm / canon_rq_pm
  shoup_forward                                 ntt_fwd_pass4, LAZY (operands below (1 + 4 stage) q, outputs below 64 q for
                                                canon_below_64q in float32) and not (below 8 q, three conditional subtractions)
  shoup_inverse                                 ntt_inv_pass4t with bd[] (4 q / 8 q / 16 q registers, sums and differences below 32 q) and
                                                ntt_inv_pass4 (4 q / 8 q); two conditional subtractions
  shoup_multiply_plain                          lazy forward passes, the lazy4 slot product, the inverse
  f64_exit                                      the last step of k_poly_f64 only: centred value -> v < 0 ? v + p : v

Operands (craft): built from an exact transform pair handed in by the caller, in the caller's own slot order -- the network's exact
transform here, the oracle on the GPU side --, so they do not depend on the kernel family that runs them.
"""
import functools
import random

import numpy as np

from galois_oracle import Q3, Q4
from test_pm_arithmetic_model import CLASSES, FOLDED, Pm, fold_pm, is_prime, mul_pm, mulvv_pm, u64

M64, M32 = (1 << 64) - 1, (1 << 32) - 1
T_PLAIN = 1 << 14
SEED = 20250


# ---- tables (csrc/host_math.h primitive_2n_root, csrc/fhe_hip.hip fhe_build_base) ------------------------------------------------------
def bitrev(x, bits):
    r = 0
    for _ in range(bits):
        r, x = (r << 1) | (x & 1), x >> 1
    return r


def primitive_2n_root(q, n):
    for g in range(2, 4096):
        c = pow(g, (q - 1) // (2 * n), q)
        if pow(c, n, q) == q - 1:
            return c
    raise ValueError("no primitive 2n-th root")


class Tables:
    def __init__(self, q, n):
        self.q, self.n, self.L = q, n, n.bit_length() - 1
        assert n == 1 << self.L and (q - 1) % (2 * n) == 0
        self.psi = primitive_2n_root(q, n)
        ipsi, self.ninv = pow(self.psi, q - 2, q), pow(n, q - 2, q)
        self.tw, self.itw = [0] * n, [0] * n
        p = ip = 1
        for j in range(n):
            r = bitrev(j, self.L)
            self.tw[r], self.itw[r] = p, ip
            p, ip = p * self.psi % q, ip * ipsi % q
        self.itw[0] = self.ninv                             # never indexed by a butterfly: n^-1
        self.itw[1] = self.itw[1] * self.ninv % q           # the last inverse stage scales its difference side
        self.twp, self.itwp = [(w << 64) // q for w in self.tw], [(w << 64) // q for w in self.itw]      # Shoup companions


@functools.lru_cache(maxsize=None)
def tables(q, n):
    return Tables(q, n)


@functools.lru_cache(maxsize=None)
def bflies(L, sigma):
    """stage sigma pairs the indices that differ in bit b = L - 1 - sigma and uses twiddle 2^sigma + (j >> (b + 1))"""
    b = L - 1 - sigma
    return [(j, j | (1 << b), (1 << sigma) + (j >> (b + 1))) for j in range(1 << L) if not (j >> b) & 1]


def pass_lo(L, P):
    return max(L - 4 * P - 4, 0)


def pass_stages(L, P):
    return min(4, L - 4 * P)


def clog(bd16):
    s = 0
    while (16 << s) < bd16:
        s += 1
    return s


def sixteenths(v, q):
    return -(-16 * v // q)


class Run:
    def __init__(self, lazy, out, reach):
        self.lazy, self.out, self.reach = lazy, out, reach


# ---- exact transforms on the same network: slot order = position in the network's output -----------------------------------------------
def exact_fwd(a, T):
    q, x = T.q, [int(v) for v in a]
    for sigma in range(T.L):
        for j0, j1, i in bflies(T.L, sigma):
            t = x[j1] * T.tw[i] % q
            x[j0], x[j1] = (x[j0] + t) % q, (x[j0] - t) % q
    return x


def exact_inv(s, T):
    q, x = T.q, [int(v) for v in s]
    for sigma in range(T.L - 1, -1, -1):
        for j0, j1, i in bflies(T.L, sigma):
            X, Y = x[j0], x[j1]
            x[j0], x[j1] = (X + Y) % q, (X - Y) * T.itw[i] % q
            if sigma == 0:
                x[j0] = x[j0] * T.ninv % q
    return x


def csub(x, q, gt=False):
    """modarith.h csub; gt: the deliberately wrong comparison `>`"""
    return x - q if (x > q if gt else x >= q) else x


# ---- pseudo-Mersenne ------------------------------------------------------------------------------------------------------------------------
def pm_fwd_bound(e0, lim, cs, stage):
    bd = e0
    for _ in range(stage):
        bd += 16 << cs
        if bd > lim:
            bd = FOLDED
    return bd


def canon_pm(v, m, gt=False):
    return csub(fold_pm(v, m), m.q, gt)


def canon_rq_pm(v, m, RQ, gt=False):
    if RQ > 32:
        v = fold_pm(v, m)
    return csub(v, m.q, gt)


def pm_forward_lazy(a, T, cls, reach, e0=16):
    """ntt_fwd_regs_pm: X' = X + T, Y' = X - T + 2^CS q; all registers folded before a stage whose bound would pass LIM"""
    c, m, q = CLASSES[cls], Pm(T.q), T.q
    off, x = q << c["CS"], [int(v) for v in a]
    for sigma in range(T.L):
        bd = pm_fwd_bound(e0, c["LIM"], c["CS"], sigma)
        if bd == FOLDED and sigma > 0 and pm_fwd_bound(e0, c["LIM"], c["CS"], sigma - 1) + (16 << c["CS"]) > c["LIM"]:
            x = [fold_pm(v, m) for v in x]
        top = topy = 0
        for j0, j1, i in bflies(T.L, sigma):
            X, Y = x[j0], x[j1]
            top, topy = max(top, X), max(topy, Y)
            t = mul_pm(Y, T.tw[i], m)
            assert 16 * t < c["RQ"] * q
            x[j0], x[j1] = u64(X + t), u64(X - t + off)
        assert bd <= c["LIM"] and 16 * max(top, topy) <= bd * q, "forward stage %d: operand above its static bound" % sigma
        reach.append(("fwd %d" % sigma, bd, sixteenths(topy, q)))
    return x


def pm_forward(a, T, cls):
    reach, m = [], Pm(T.q)
    lazy = pm_forward_lazy(a, T, cls, reach)
    return Run(lazy, [canon_pm(v, m) for v in lazy], reach)


def pm_inv_plan(L, P, EB, c):
    """ntt_core.h pm_inv_plan, per register index of the pass; also the static bound of every difference and sum"""
    LO, S = pass_lo(L, P), pass_stages(L, P)
    LIM, RQ, XB = c["LIM"], c["RQ"], c["XB"]
    bd, pl = [EB] * 16, {}
    for u in range(S - 1, -1, -1):
        sigma = 4 * P + u
        rb = (L - 1 - sigma) - LO
        for r0 in range(16):
            if r0 & (1 << rb):
                continue
            r1 = r0 | (1 << rb)
            fy = fx = False
            if bd[r0] + (16 << clog(bd[r1])) > LIM:
                fy, bd[r1] = True, FOLDED
            if bd[r0] + (16 << clog(bd[r1])) > LIM:
                fx, bd[r0] = True, FOLDED
            sh = clog(bd[r1])
            pl[(u, r0)] = (fy, fx, sh, bd[r0] + (16 << sh), bd[r0] + bd[r1])
            bd[r0] = RQ if sigma == 0 else bd[r0] + bd[r1]
            bd[r1] = RQ
    return pl, [P > 0 and bd[r] > XB for r in range(16)], bd


def pm_inverse_lazy(s, T, cls, reach, e0=16):
    """ntt_inv_regs_pm: T = X + Y unreduced, D = X - Y + 2^shift q through the product; operands folded where the plan says so"""
    c, m, q, L = CLASSES[cls], Pm(T.q), T.q, T.L
    x, NP = [int(v) for v in s], (L + 3) // 4
    assert all(16 * v <= e0 * q for v in x)
    for P in range(NP - 1, -1, -1):
        LO = pass_lo(L, P)
        pl, fold_exit, bd_out = pm_inv_plan(L, P, e0 if P == NP - 1 else c["XB"], c)
        for u in range(pass_stages(L, P) - 1, -1, -1):
            sigma, top, topb = 4 * P + u, 0, 0
            for j0, j1, i in bflies(L, sigma):
                fy, fx, sh, dbd, tbd = pl[(u, (j0 >> LO) & 15)]
                X, Y = x[j0], x[j1]
                if fy:
                    Y = fold_pm(Y, m)
                if fx:
                    X = fold_pm(X, m)
                t, d = u64(X + Y), u64(X - Y + (q << sh))
                assert dbd <= c["LIM"] and 16 * d <= dbd * q and 16 * t <= tbd * q, "inverse stage %d: operand above its static bound" % sigma
                top, topb = max(top, d), max(topb, dbd)
                if sigma == 0:
                    assert tbd <= c["LIM"]
                    top = max(top, t)
                    x[j0] = mul_pm(t, T.ninv, m)
                else:
                    x[j0] = t
                x[j1] = mul_pm(d, T.itw[i], m)
                assert 16 * x[j1] < c["RQ"] * q
            reach.append(("inv %d" % sigma, topb, sixteenths(top, q)))
        for j in range(1 << L):
            r = (j >> LO) & 15
            if fold_exit[r]:
                x[j] = fold_pm(x[j], m)
            assert 16 * x[j] <= (FOLDED if fold_exit[r] else bd_out[r]) * q
            assert 16 * x[j] <= (c["XB"] if P > 0 else c["RQ"]) * q
    return x


def pm_inverse(s, T, cls):
    reach, m = [], Pm(T.q)
    lazy = pm_inverse_lazy(s, T, cls, reach)
    return Run(lazy, [canon_rq_pm(v, m, CLASSES[cls]["RQ"]) for v in lazy], reach)


def pm_multiply_plain(a, w_slots, T, cls):
    """k_mulplain_pm: forward -> mulvv_pm(fold_pm(.), w) with the plaintext's canonical slot values -> inverse entered below RQ"""
    reach, m, c = [], Pm(T.q), CLASSES[cls]
    f = pm_forward_lazy(a, T, cls, reach)
    y = []
    for v, w in zip(f, w_slots):
        p = mulvv_pm(fold_pm(v, m), int(w), m)              # asserts a < 2^(b+1), w canonical
        assert 16 * p <= c["RQ"] * T.q
        y.append(p)
    lazy = pm_inverse_lazy(y, T, cls, reach, e0=c["RQ"])
    return Run(lazy, [canon_rq_pm(v, m, c["RQ"]) for v in lazy], reach)


# ---- Shoup with the approximate high word (modarith.h) ------------------------------------------------------------------------------------
def mul_shoup_lazy4(x, w, wp, q, acc=0):
    """mul_shoup_lazy4 / mul_shoup_lazy4_acc as written: the high word of x wp without the low x low partial product and without the
    carries of the cross terms (but with the carry of their sum), the subtraction as an addition of qhat (2^64 - q), the high word of
    the result from one three-operand add.  Any 64-bit x; returns acc + (x w mod q + {0, 1, 2} q)."""
    u64(x), u64(acc)
    xl, xh, wl, wh, pl, ph = x & M32, x >> 32, w & M32, w >> 32, wp & M32, wp >> 32
    s = ((xh * pl) >> 32) + ((xl * ph) >> 32)               # __builtin_addc of the two v_mul_hi_u32
    cy, s = s >> 32, s & M32
    A = u64(xh * ph + ((cy << 32) | s))
    al, ah, nq = A & M32, A >> 32, (1 << 64) - q
    nl, nh = nq & M32, nq >> 32
    P = (al * nl + (xl * wl + acc)) & M64                   # two wrapping v_mad_u64_u32
    Cc = (ah * nl + (al * nh + (xh * wl + xl * wh))) & M64
    hi = ((P >> 32) + (Cc & M32)) & M32                     # v_add3_u32; the third addend is anded with the opaque zero
    r = (hi << 32) | (P & M32)
    exact = (x * w) // q
    # x wp / 2^64 falls short of x w / q by x eps / 2^64 < 1, the three dropped fractions by less than 3: exact - 3 <= A.  (modarith.h says
    # "exact - 2"; a shortfall of 3 occurs in about 0.2 % of random products.  The RANGE it states, [0, 4q), is what the passes use, and holds.)
    assert exact - 3 <= A <= exact, "quotient estimate outside [exact - 3, exact]"
    assert 0 <= x * w - A * q < 4 * q and r == acc + x * w - A * q, "lazy4 product outside [0, 4q) or wrapped"
    return r


def canon_scale(q, factor=True):
    """ntt_core.h canon_scale: (float)((2^32 / (double)q) (1 - 2^-17)); factor=False: the deliberately wrong constant"""
    return np.float32((4294967296.0 / float(q)) * ((1.0 - 2.0 ** -17) if factor else 1.0))


def canon_below_64q(v, q, c, strict=True):
    """three roundings (u32 -> float, the constant, the product) and the truncation, in numpy float32"""
    qhat = int(np.float32(v >> 32) * c)
    d = v - qhat * q
    if strict:
        assert v < 64 * q and 0 <= qhat <= M32 and 0 <= d < 2 * q, "canon_below_64q: estimate outside {Q - 1, Q}"
    return csub(d & M64, q)


def exit_fwd_nolazy(v, q, gt=-1):
    """csub(csub(csub(x, 4q), 2q), q); gt = the index of the comparison written `>`"""
    return csub(csub(csub(v, 4 * q, gt == 0), 2 * q, gt == 1), q, gt == 2)


def exit_inv(v, q, gt=-1):
    return csub(csub(v, 2 * q, gt == 0), q, gt == 1)


def shoup_forward_lazy(a, T, lazy, reach):
    """ntt_fwd_pass4: S = X + T from the product's accumulator, Y' = 2X + 4q - S; LAZY: no conditional subtraction, +4q per stage"""
    q, x = T.q, [int(v) for v in a]
    q4 = 4 * q
    for sigma in range(T.L):
        bd, top = (16 * (1 + 4 * sigma) if lazy else 128), 0
        for j0, j1, i in bflies(T.L, sigma):
            top = max(top, x[j0], x[j1])
            X = x[j0] if lazy else csub(x[j0], q4)
            S = mul_shoup_lazy4(x[j1], T.tw[i], T.twp[i], q, X)
            x[j0], x[j1] = S, u64((X << 1) + q4 - S)
        assert 16 * top < bd * q, "forward stage %d: operand above its bound" % sigma
        reach.append(("fwd %d" % sigma, bd, sixteenths(top, q)))
    return x


def shoup_forward(a, T, lazy):
    reach, q = [], T.q
    v = shoup_forward_lazy(a, T, lazy, reach)
    if lazy:
        assert 2 ** 33 <= q < 2 ** 58
        c = canon_scale(q)
        reach.append(("canon", 16 * 64, sixteenths(max(v), q)))
        return Run(v, [canon_below_64q(e, q, c) for e in v], reach)
    assert all(e < 8 * q for e in v)
    return Run(v, [exit_fwd_nolazy(e, q) for e in v], reach)


def shoup_inverse_lazy(s, T, lazy, reach):
    """lazy: ntt_inv_pass4t (primes <= 58 bits, the bound of every register tracked as bd[] in units of q); else ntt_inv_pass4"""
    q, L = T.q, T.L
    x, NP, q4 = [int(v) for v in s], (L + 3) // 4, 4 * q
    assert all(v < q4 for v in x)
    if lazy:
        assert 32 * q <= M64
    for P in range(NP - 1, -1, -1):
        LO = pass_lo(L, P)
        bd = [4 if P == NP - 1 else 8] * 16
        for u in range(pass_stages(L, P) - 1, -1, -1):
            sigma, top = 4 * P + u, 0
            rb = (L - 1 - sigma) - LO
            for j0, j1, i in bflies(L, sigma):
                X, Y = x[j0], x[j1]
                if lazy:
                    r0 = (j0 >> LO) & 15
                    r1 = r0 | (1 << rb)
                    assert X < bd[r0] * q and Y < bd[r1] * q and bd[r1] in (4, 8, 16)
                    t, d = u64(X + Y), u64(X - Y + bd[r1] * q)
                    assert t < 32 * q and 0 < d < 32 * q
                    if sigma and bd[r0] + bd[r1] > 16:
                        t = csub(t, 16 * q)
                        assert t < 16 * q
                else:
                    assert X < q4 and Y < q4
                    t, d = csub(X + Y, q4), u64(X - Y + q4)
                top = max(top, d)
                x[j0] = mul_shoup_lazy4(t, T.itw[0], T.itwp[0], q) if sigma == 0 else t
                x[j1] = mul_shoup_lazy4(d, T.itw[i], T.itwp[i], q)
            if lazy:                                          # the bounds after the stage, as the unrolled kernel knows them
                nb = list(bd)
                for r0 in range(16):
                    if not r0 & (1 << rb):
                        r1 = r0 | (1 << rb)
                        nb[r0], nb[r1] = (4 if sigma == 0 else min(bd[r0] + bd[r1], 16)), 4
                bd = nb
            reach.append(("inv %d" % sigma, 16 * (32 if lazy else 8), sixteenths(top, q)))
        if lazy and P > 0:
            for j in range(1 << L):
                if bd[(j >> LO) & 15] > 8:
                    x[j] = csub(x[j], 8 * q)
                assert x[j] < 8 * q
    assert all(v < q4 for v in x)
    return x


def shoup_inverse(s, T, lazy):
    reach = []
    v = shoup_inverse_lazy(s, T, lazy, reach)
    return Run(v, [exit_inv(e, T.q) for e in v], reach)


def shoup_multiply_plain(a, w_slots, T, lazy):
    """k_mulplain<L, LAZY>: LAZY is decided by the widest prime alone (<= 58 bits); the slot product takes any 64-bit operand"""
    reach, q = [], T.q
    f = shoup_forward_lazy(a, T, lazy, reach)
    y = [mul_shoup_lazy4(v, int(w), (int(w) << 64) // q, q) for v, w in zip(f, w_slots)]
    v = shoup_inverse_lazy(y, T, lazy, reach)
    return Run(v, [exit_inv(e, q) for e in v], reach)


# ---- FP64: the last step only ----------------------------------------------------------------------------------------------------------------
def centred(r, q):
    """what the exact-FP64 kernels hold before their last step: the representative of least absolute value"""
    return r if r <= q // 2 else r - q


def f64_exit(c, q, le=False):
    """v < 0.0 ? v + p : v; le: the deliberately wrong `<=`"""
    return c + q if (c <= 0 if le else c < 0) else c


# ---- bases -------------------------------------------------------------------------------------------------------------------------------------
def largest_primes(bits, n, count=2):
    """the largest `count` primes of `bits` bits that are 1 (mod 2n)"""
    out, m = [], (1 << bits) + 1
    while len(out) < count:
        m -= 2 * n
        if is_prime(m):
            out.append(m)
    assert all(p.bit_length() == bits for p in out)
    return out


NOPM, NOLAZY, SINGLE, FORCE_U64 = {"FHE_NTT_NOPM": 1}, {"FHE_NTT_NOLAZY": 1}, {"FHE_NTT_SINGLE": 1}, {"FHE_DCT_FORCE_U64": 1}


def base(name, n):
    """name -> (q, plain modulus, switches, fhe_arith_path & 3, model family, forward/inverse transforms lazy, multiply_plain lazy)"""
    if name == "pm-A":
        return Q4, T_PLAIN, {}, 1, "A", None, None
    if name == "pm-B":
        return largest_primes(58, n), T_PLAIN, {}, 2, "B", None, None
    if name == "shoup-lazy-A":
        return Q4, T_PLAIN, dict(NOPM), 0, "shoup", True, True
    if name == "shoup-lazy-B":
        return largest_primes(58, n), T_PLAIN, dict(NOPM), 0, "shoup", True, True
    if name == "shoup-small":                                  # the 36/37-bit P4096 primes below the FP64 kernels' n
        return Q3, T_PLAIN, {}, 0, "shoup", True, True
    if name == "shoup-nolazy-61":
        return largest_primes(61, n, 1) + largest_primes(60, n, 1), T_PLAIN, {}, 0, "shoup", False, False
    if name == "shoup-nolazy-A":                                # multiply_plain keeps its lazy kernel: only the prime width decides there
        return Q4, T_PLAIN, dict(NOPM, **NOLAZY), 0, "shoup", False, True
    if name == "shoup-nolazy-33":                               # below 2^33 canon_below_64q is not used: the transforms are not lazy
        return largest_primes(33, n), 1 << 10, dict(FORCE_U64), 0, "shoup", False, True
    if name == "fp64":
        return Q3, T_PLAIN, {}, 0, "f64", None, None
    raise KeyError(name)


def model(family, T, tf_lazy=None, mp_lazy=None):
    """(forward, inverse, multiply_plain) models of one prime"""
    if family in ("A", "B"):
        return (lambda a: pm_forward(a, T, family)), (lambda s: pm_inverse(s, T, family)), (lambda a, w: pm_multiply_plain(a, w, T, family))
    return (lambda a: shoup_forward(a, T, tf_lazy)), (lambda s: shoup_inverse(s, T, tf_lazy)), (lambda a, w: shoup_multiply_plain(a, w, T, mp_lazy))


def exit_bound(family, op, q, L, lazy=None):
    """the range the value in front of the canonicalisation lies in, from the kernels' own range statements: a target r can appear as
    r + q or more only when r + q is below this"""
    if family in ("A", "B"):
        m = Pm(q)
        if op == "fwd":
            return pm_fwd_bound(16, CLASSES[family]["LIM"], CLASSES[family]["CS"], L) * q // 16
        return (1 << m.b) + (m.delta << 32)                 # mul_pm's result
    if op == "fwd":
        return (1 + 4 * L) * q if lazy else 8 * q
    return 4 * q


# ---- operands ------------------------------------------------------------------------------------------------------------------------------------
def targets(q):
    return [0, 1, 2, q // 2, q // 2 + 1, q - 2, q - 1]


def pattern(q, n, kind, seed):
    """mixed: half of the positions drawn from the targets, the rest random; dense: every position; each target in >= n/32 positions"""
    rng, V = random.Random("%d/%d/%s/%d" % (q, n, kind, seed)), targets(q)
    count = n if kind == "dense" else n // 2
    vals = [V[i % 7] for i in range(count)]
    rng.shuffle(vals)
    out = [rng.randrange(q) for _ in range(n)]
    for p, v in zip(rng.sample(range(n), count), vals):
        out[p] = v
    assert all(sum(1 for v in out if v == t) >= n // 32 for t in V)
    return out


def structured(q, n):
    out = [("all q-1", [q - 1] * n), ("all q/2", [q // 2] * n), ("0, q-1 alternating", [0, q - 1] * (n // 2))]
    for j in (0, 1, n // 2, n - 1):
        out.append(("(q-1) X^%d" % j, [(q - 1) if i == j else 0 for i in range(n)]))
    return out


def inv_all(vals, q):
    """element-wise inverses with one modular exponentiation"""
    pre, acc = [], 1
    for v in vals:
        pre.append(acc)
        acc = acc * v % q
    inv, out = pow(acc, q - 2, q), [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        out[i] = inv * pre[i] % q
        inv = inv * vals[i] % q
    return out


class Crafted:
    """operands of one base at one n.  F: forward inputs (coefficients) and their exact slots F_slots (the caller's slot order); I: inverse
    inputs (slots, the caller's order) and their exact outputs I_out; M: multiply_plain inputs with exact outputs M_out, the plaintext
    `plain` and its slot values P_slots.  Arrays are uint64 [polynomial][prime][n]; *_names label the polynomials; *_pat[name] = the
    prescribed pattern of a crafted polynomial ([prime][n])."""


def craft(q, n, t, fwd, inv, seed=SEED):
    """fwd(i, coefficients) / inv(i, slots): exact transforms modulo q[i] on lists of Python integers, one consistent slot order"""
    k, cr = len(q), Crafted()
    rng = random.Random("plain/%d/%d" % (n, seed))
    while True:                                              # small non-negative coefficients: the lift is the identity
        plain = [rng.randrange(1, t // 2) for _ in range(n)]
        P_slots = [fwd(i, [c % q[i] for c in plain]) for i in range(k)]
        if all(all(P_slots[i]) for i in range(k)):
            break
    pats = {kind: [pattern(q[i], n, kind, seed) for i in range(k)] for kind in ("mixed", "dense")}
    F, I, M = [], [], []
    for kind in ("mixed", "dense"):
        F.append((kind, [inv(i, pats[kind][i]) for i in range(k)]))
        I.append((kind, [fwd(i, pats[kind][i]) for i in range(k)]))
        M.append(("out " + kind, [inv(i, [a * b % q[i] for a, b in zip(fwd(i, pats[kind][i]), inv_all(P_slots[i], q[i]))]) for i in range(k)]))
    for kind in ("mixed", "dense"):
        M.append(("mid " + kind, [inv(i, pats[kind][i]) for i in range(k)]))
    st = [structured(q[i], n) for i in range(k)]
    for j in range(len(st[0])):
        row = (st[0][j][0], [st[i][j][1] for i in range(k)])
        F.append(row), I.append(row), M.append(row)
    arr = lambda rows: np.array([[[int(v) for v in p] for p in r[1]] for r in rows], dtype=np.uint64)
    cr.q, cr.n, cr.t, cr.k = list(q), n, t, k
    cr.plain, cr.P_slots = np.array(plain, dtype=np.uint64), np.array(P_slots, dtype=np.uint64)
    cr.F_names, cr.I_names, cr.M_names = [r[0] for r in F], [r[0] for r in I], [r[0] for r in M]
    cr.F, cr.I, cr.M = arr(F), arr(I), arr(M)
    cr.F_slots = arr([(nm, [fwd(i, p[i]) for i in range(k)]) for nm, p in F])
    cr.I_out = arr([(nm, [inv(i, p[i]) for i in range(k)]) for nm, p in I])
    cr.M_out = arr([(nm, [inv(i, [a * b % q[i] for a, b in zip(fwd(i, p[i]), P_slots[i])]) for i in range(k)]) for nm, p in M])
    P = np.array([pats["mixed"], pats["dense"]], dtype=np.uint64)
    cr.F_pat = {"mixed": P[0], "dense": P[1]}                 # forward: the slots; inverse: the coefficients
    cr.M_pat = {"out mixed": P[0], "out dense": P[1], "mid mixed": P[0], "mid dense": P[1]}      # out: the product; mid: the forward slots
    for j, nm in enumerate(("mixed", "dense")):
        assert np.array_equal(cr.F_slots[j], P[j]) and np.array_equal(cr.I_out[j], P[j]) and np.array_equal(cr.M_out[j], P[j])
    return cr


@functools.lru_cache(maxsize=None)
def crafted_by_model(name, n):
    """the operands of base `name` built with the network's own exact transforms: the arrays tests/test_ntt_craft_cpu.py analyses and,
    at n = 1024, the ones tests/test_gpu_ntt_extremes.py runs"""
    q, t = base(name, n)[:2]
    return craft(q, n, t, lambda i, a: exact_fwd(a, tables(q[i], n)), lambda i, s: exact_inv(s, tables(q[i], n)))


def slot_permutation(src_x, dst_x):
    """Two exact transforms of the monomial X hold the same n distinct odd powers of a primitive 2n-th root, each in its own slot order:
    perm[s] = the position in `dst` of the slot at position s in `src`; asserted to be a bijection."""
    where = {int(v): p for p, v in enumerate(dst_x)}
    assert len(where) == len(dst_x), "the slots of X are not distinct"
    perm = np.array([where.get(int(v), -1) for v in src_x], dtype=np.int64)
    assert perm.min() >= 0 and len(set(perm.tolist())) == len(src_x), "no bijection between the two slot orders"
    return perm
