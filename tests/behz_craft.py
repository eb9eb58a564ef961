"""A scalar big-integer restatement of the BEHZ ciphertext product (csrc/behz.hip, steps 0, 1, 3 and 4) for ONE coefficient, the
library's choice of auxiliary base restated from fhe_behz_build, and operands crafted with both so that chosen coefficients put
chosen values under the kernels' base conversions.  No GPU imports; tests/test_behz_craft_cpu.py proves in the model that every
target is reached, tests/test_gpu_behz_extremes.py runs the operands through the kernels.

The steps, for a coefficient with residues a_i (m~ = 2^32, q = prod q_i, Bsk = {b_0 .. b_(k-1), m_sk}, B = prod b_j):
  0   y_i = [m~ a_i (q/q_i)^-1]_{q_i}                    canonical, used as an integer:  x = sum y_i (q/q_i)
  1   r = [-x q^-1]_{m~}, centred (r >= 2^31 counts as r - 2^32);  lift = (x + q r) / m~   -- congruent to a (mod q), in [-q/2, q/2 + k q / 2^32)
  2   D = sum of negacyclic products of lifts (exact integers here)
  3   y_i = [t D (q/q_i)^-1]_{q_i};  v = (t D - sum y_i (q/q_i)) / q;  f_j = [v]_{b_j}, f_sk = [v]_{m_sk}
  4   z_j = [f_j (B/b_j)^-1]_{b_j};  conv = sum z_j (B/b_j) = v + alpha B;  alpha_sk = [(conv - f_sk) B^-1]_{m_sk}, centred;
      result_i = [conv - alpha_sk B]_{q_i}  = [v]_{q_i} as long as |alpha| < m_sk / 2
The kernels split y_i at 2^28 (PM_SPLIT_Y) or 2^29 (Dot58), z_j and |alpha_sk| at 2^29 (PM_SPLIT_Z), and branch on r >= 2^31.

Why single coefficients can be aimed at.  Steps 0 and 1 are per coefficient.  lift(a) is congruent to a (mod q), so the residues
of D -- and with them the y_i of step 3 -- are free by CRT when the other operand is the constant polynomial 1; and when the other
operand is (c, 0) -- a constant c = 2^s and a zero polynomial -- output coefficient j of polynomial p is lift(a_p[j]) c and nothing else,
so every coefficient is a scalar BEHZ case of its own.  With t c >= 4 max b_j the floor value v sweeps more than a whole b_j
while |a'| stays below q / 4, where lift(a' mod q) == a' (floor_constant)."""
import random

import numpy as np

from galois_oracle import Q4, T_BATCH as T_PRIME
from oracle.bigint_model import polymul_negacyclic, prod
from oracle.oracle import PRESETS
from slot_craft import is_prime

MT = 1 << 32
M32 = MT - 1
SPLIT_Y, SPLIT_Z = 28, 29                # PM_SPLIT_Y; PM_SPLIT_Z and the 29-bit halves of Dot58 (csrc/behz.hip)
R_TARGETS = (0, 1, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFF)
LIFT_VARIANTS, FLOOR_VARIANTS = ("centre_gt", "lift_y_keeps_q"), ("floor_y_keeps_q", "alpha_byte")      # deliberately wrong models: see Scalar
VARIANTS = LIFT_VARIANTS + FLOOR_VARIANTS

SMALL_Q = PRESETS["P4096"]["q"]                                # 36/37 bits; SMALL of tests/test_gpu_parity.py at n = 1024
T_POW2 = 1 << 14


def primes_below(bits, count, step=1 << 17, skip=()):
    """the largest `count` primes = 1 (mod step) below 2^bits that are not in `skip`, descending"""
    out, cand = [], (1 << bits) + 1 - step
    while len(out) < count:
        if is_prime(cand) and cand not in skip:
            out.append(cand)
        cand -= step
    return out


Q61X5 = primes_below(61, 5)              # five 61-bit primes = 1 (mod 2^17): the boundary base; they are the first candidates of a 61-bit auxiliary base too

# name -> (n, q, t): the contexts of tests/test_gpu_behz_extremes.py
BASES = {name: (PRESETS[name]["n"], PRESETS[name]["q"], PRESETS[name]["t"]) for name in ("SEAL23_4096", "P8192", "SEAL23_2048", "SEAL23_16384")}
BASES.update({
    "SMALL": (1024, SMALL_Q, T_POW2),
    "Q4-prime-t": (1024, Q4, T_PRIME),
    "Q61x5-n1024": (1024, Q61X5, T_POW2),
    "Q61x5-n2048": (2048, Q61X5, T_POW2),
})


def aux_need(q, t, n):
    """the bits the auxiliary base has to offer (fhe_behz_build): bits(q) + bits(t) + log2 n + 8 (sizes up to 2^8) + 4"""
    return sum(p.bit_length() for p in q) + t.bit_length() + (n.bit_length() - 1) + 12


def library_aux(q, t, n, aux61=False):
    """fhe_behz_build restated: 58-bit auxiliary primes when 57 (k + 1) bits are enough (and FHE_BEHZ_AUX61 is not set), else
    61-bit ones; descending from 2^bits in steps of 2^17, skipping the q_i; the first prime found is m_sk, the next k form B"""
    k = len(q)
    bits = 58 if 57 * (k + 1) >= aux_need(q, t, n) and not aux61 else 61
    found = primes_below(bits, k + 1, skip=set(q))
    return dict(bits=bits, msk=found[0], b=found[1:])


def seal_aux(q):
    """the 61-bit base of SEAL 2.3 and of the C oracle"""
    found = primes_below(61, len(q) + 1, skip=set(q))
    return dict(bits=61, msk=found[0], b=found[1:])


class Scalar:
    """Steps 0/1 (lift) and 3/4 (floor) for one coefficient, in Python integers, through the auxiliary base `aux`.

    variant: None, or one deliberately wrong restatement; LIFT_VARIANTS change lift() only, FLOOR_VARIANTS floor() only
      centre_gt         step 1 centres with r > 2^31 where the kernels test r >= 2^31: wrong by a whole q exactly at r = 0x80000000
      lift_y_keeps_q    step 0 leaves y_i = q_i where the canonical value is 0: x grows by q and r drops by one, which cancels unless
                        r steps across the centring boundary (r = 0x80000000 with some y_i = 0; needs k >= 2: with one prime y_0 = 0 is a = 0)
      floor_y_keeps_q   step 3 leaves y_i = q_i where the canonical value is 0: the fast floor is off by one
      alpha_byte        step 4 keeps alpha_sk as a signed byte -- room for the |alpha_sk| <= k that holds for SMALL floor values only;
                        alpha_sk is about -v / B, thousands to millions for a product of full-size operands
    The first three are invisible to random data of any kind (events of probability 2^-32 or 2^-36 .. 2^-61 per coefficient).
    alpha_byte is invisible only to random coefficients against the scalar operands (1, 0) and (c, 0), where |v| <= 2 b_j: a product
    of two random ciphertexts has |alpha_sk| in the hundreds or thousands wherever q outgrows B, so the random parity tests do see
    it.  It is kept as the model of the false "|alpha_sk| <= k" that stood in the kernels' comments, not as a mistake only crafted
    data finds; on the single-prime base, where lift_y_keeps_q cannot apply, it is the third variant with that caveat.
    Not among them: a split that drops a bit of a high half (whatever bit it is, it is set in half of all random y_i or z_j, so random
    data sees it), a canonicalisation that leaves b_j in place of z_j = 0 (no data sees it: conv grows by B and alpha_sk by one, the
    result is the same) and one that leaves q_i in place of a result 0 (every zero operand shows it; test_gpu_parity.py multiplies one)."""

    def __init__(self, q, t, aux, variant=None):
        assert variant is None or variant in VARIANTS
        self.q, self.t, self.k, self.variant = list(q), t, len(q), variant
        self.b, self.msk = list(aux["b"]), aux["msk"]
        assert len(self.b) == self.k
        self.Q, self.B = prod(self.q), prod(self.b)
        self.punct = [self.Q // p for p in self.q]
        self.inv_punct = [pow(m, -1, p) for m, p in zip(self.punct, self.q)]
        self.mt_inv_punct = [MT * w % p for w, p in zip(self.inv_punct, self.q)]
        self.t_inv_punct = [t * w % p for w, p in zip(self.inv_punct, self.q)]
        self.punct_mod_mt = [m & M32 for m in self.punct]
        self.neg_inv_q_mt = (-pow(self.Q, -1, MT)) % MT
        self.punct_B = [self.B // p for p in self.b]
        self.inv_punct_B = [pow(m, -1, p) for m, p in zip(self.punct_B, self.b)]
        self.inv_B_msk = pow(self.B, -1, self.msk)

    # -- steps 0 + 1 ------------------------------------------------------------------------------------------------------
    def lift(self, a):
        """a: the k residues of one coefficient -> dict(value, y, r); r is the remainder as the kernels hold it, in [0, 2^32)"""
        y = [x * w % p for x, w, p in zip(a, self.mt_inv_punct, self.q)]
        if self.variant == "lift_y_keeps_q":
            y = [p if v == 0 else v for v, p in zip(y, self.q)]
        r = ((sum((v & M32) * m for v, m in zip(y, self.punct_mod_mt)) & M32) * self.neg_inv_q_mt) & M32
        negative = r > 0x80000000 if self.variant == "centre_gt" else r >= 0x80000000
        num = sum(v * m for v, m in zip(y, self.punct)) + self.Q * (r - MT if negative else r)
        assert num % MT == 0
        return dict(value=num // MT, y=y, r=r)

    def y_for(self, target, which):
        """the residue a_i that gives y_i = target in step 0 (which = "lift") or, for D = a (mod q_i), in step 3 (which = "floor")"""
        w = self.mt_inv_punct if which == "lift" else self.t_inv_punct
        return [v * pow(x, -1, p) % p for v, x, p in zip(target, w, self.q)]

    # -- steps 3 + 4 ------------------------------------------------------------------------------------------------------
    def floor(self, D):
        """D: the integer coefficient of the tensor sum -> dict(result, y, v, f, z, alpha)"""
        y = [(self.t * D % p) * w % p for w, p in zip(self.inv_punct, self.q)]
        if self.variant == "floor_y_keeps_q":
            y = [p if v == 0 else v for v, p in zip(y, self.q)]
        num = self.t * D - sum(v * m for v, m in zip(y, self.punct))
        assert num % self.Q == 0
        v = num // self.Q
        f = [v % p for p in self.b] + [v % self.msk]
        z = [x * w % p for x, w, p in zip(f, self.inv_punct_B, self.b)]
        conv = sum(x * m for x, m in zip(z, self.punct_B))
        alpha = (conv - f[self.k]) * self.inv_B_msk % self.msk
        if alpha > self.msk >> 1:
            alpha -= self.msk
        if self.variant == "alpha_byte":
            alpha = (alpha + 128) % 256 - 128
        res = [(conv - alpha * self.B) % p for p in self.q]
        return dict(result=res, y=y, v=v, f=f, z=z, alpha=alpha)

    def coefficient(self, a, c):
        """one coefficient of multiply(a, (c, 0)): (lift info, floor info)"""
        lf = self.lift(a)
        return lf, self.floor(lf["value"] * c)

    # -- whole products: scalar steps around an exact integer convolution -----------------------------------------------------
    def lift_poly(self, poly):
        """poly [k][n] uint64 -> list of n lift infos"""
        return [self.lift(list(col)) for col in zip(*[row.tolist() for row in poly])]

    def multiply(self, a, b):
        """a [sa][k][n], b [sb][k][n] uint64 -> (result [sa + sb - 1][k][n] uint64, floor info per [polynomial][coefficient])"""
        n = a.shape[-1]
        al = [[x["value"] for x in self.lift_poly(p)] for p in a]
        bl = al if b is a else [[x["value"] for x in self.lift_poly(p)] for p in b]
        D = [[0] * n for _ in range(len(al) + len(bl) - 1)]
        for i, x in enumerate(al):
            if not any(x):
                continue
            for j, y in enumerate(bl):
                if any(y):
                    D[i + j] = [u + w for u, w in zip(D[i + j], polymul_negacyclic(x, y))]
        return self.floor_polys(D)

    def floor_polys(self, D):
        info = [[self.floor(d) for d in poly] for poly in D]
        out = np.array([[[x["result"][i] for x in poly] for i in range(self.k)] for poly in info], dtype=np.uint64)
        return out, info


# ---------------------------------------------------------------------------------------------------------------------------
# targets and labels
# ---------------------------------------------------------------------------------------------------------------------------
def y_points(p):
    """name -> value: the points of a y_i (or, with p = b_j, of a z_j) the kernels can get wrong"""
    return {"0": 0, "1": 1, "m-2": p - 2, "m-1": p - 1, "2^28-1": (1 << 28) - 1, "2^28": 1 << 28, "2^29-1": (1 << 29) - 1, "2^29": 1 << 29}


Z_POINTS = ("0", "1", "m-2", "m-1", "2^29-1", "2^29")


def lift_targets(k):
    return (["lift.y%d=%s" % (i, nm) for i in range(k) for nm in y_points(1 << 40)] + ["lift.all=m-1", "lift.all=0"] +
            ["lift.r=0x%08X" % r for r in R_TARGETS] + (["lift.y0=0&r=0x80000000"] if k > 1 else []))


def floor_y_targets(k):
    return ["floor.y%d=%s" % (i, nm) for i in range(k) for nm in y_points(1 << 40)] + ["floor.all=m-1", "floor.all=0", "floor.v>=0", "floor.v<0"]


def _z_star(sc, j, nm, sign):
    """the floor value that gives z_j the named point: v* = z* (B/b_j) mod b_j, or v* - b_j for a negative one"""
    return y_points(sc.b[j])[nm] * sc.punct_B[j] % sc.b[j] - (sc.b[j] if sign == "<0" else 0)


def floor_constant(q, t, aux):
    """c = 2^s of the operand (c, 0) that most z_j cases share: the smallest with t c >= 4 max b_j, so that v sweeps more than a whole
    b_j in both directions while |a'| < q / 4 -- but never beyond t c <= q / 4, where consecutive a' stop reaching consecutive v (a base
    of one 54-bit prime: there the shared sweep is +-2^50, short of b_j, and the far targets get constants of their own: floor_z_extra_cases)"""
    s, Q = 0, prod(q)
    while (t << s) < 4 * max(aux["b"]) and (t << (s + 1)) <= Q // 4:
        s += 1
    return 1 << s


def floor_z_targets(q, t, aux, shared=None):
    """every (z_j, point, sign of v): 12 k targets.  shared=True: those whose floor value lies inside the sweep |v*| <= t c / 4 of the
    shared constant (all of them when q has 62 bits -- 65 with 61-bit auxiliary primes); shared=False: the others"""
    sc, c = Scalar(q, t, aux), floor_constant(q, t, aux)
    return ["floor.z%d=%s,v%s" % (j, nm, sg) for j in range(sc.k) for nm in Z_POINTS for sg in (">=0", "<0")
            if shared is None or (abs(_z_star(sc, j, nm, sg)) <= t * c // 4) == shared]


def _parse_z(sc, label):
    zj, sign = label[len("floor."):].split(",v")
    return _z_star(sc, int(zj[1:zj.index("=")]), zj[zj.index("=") + 1:], sign)


def labels_of(lf, fl, sc):
    """the targets one coefficient hits, read off the model's intermediates (never off what a builder meant to do)"""
    out = set()
    for stage, ys in (("lift", lf["y"] if lf else None), ("floor", fl["y"] if fl else None)):
        if ys is None:
            continue
        for i, (v, p) in enumerate(zip(ys, sc.q)):
            for nm, val in y_points(p).items():
                if v == val:
                    out.add("%s.y%d=%s" % (stage, i, nm))
        if all(v == p - 1 for v, p in zip(ys, sc.q)):
            out.add("%s.all=m-1" % stage)
        if all(v == 0 for v in ys):
            out.add("%s.all=0" % stage)
    if lf and lf["r"] in R_TARGETS:
        out.add("lift.r=0x%08X" % lf["r"])
        out |= {"lift.y%d=0&r=0x80000000" % i for i, v in enumerate(lf["y"]) if v == 0 and lf["r"] == 0x80000000}
    if fl:
        sg = ">=0" if fl["v"] >= 0 else "<0"
        out.add("floor.v" + sg)
        for j, (v, p) in enumerate(zip(fl["z"], sc.b)):
            pts = y_points(p)
            for nm in Z_POINTS:
                if v == pts[nm]:
                    out.add("floor.z%d=%s,v%s" % (j, nm, sg))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# builders: operands in the library's [poly][k][n] layout and {(poly, coefficient): label}
# ---------------------------------------------------------------------------------------------------------------------------
def random_poly(q, n, rng):
    return np.stack([rng.integers(0, p, size=n, dtype=np.uint64) for p in q])


def _place(q, n, cases, seed):
    """a size-2 operand: polynomial 0 holds the cases from coefficient 0 upwards, polynomial 1 the same cases from coefficient n - 1
    downwards (other lanes, the other coefficient of a thread); every other coefficient is seeded random padding"""
    assert len(cases) <= n
    rng = np.random.default_rng(seed)
    a = np.stack([random_poly(q, n, rng), random_poly(q, n, rng)])
    labels = {}
    for idx, (label, res) in enumerate(cases):
        for poly, pos in ((0, idx), (1, n - 1 - idx)):
            a[poly, :, pos] = np.array(res, dtype=np.uint64)
            labels[(poly, pos)] = label
    return a, labels


def constant_ct(q, n, c):
    """(c, 0): the constant polynomial c and a zero polynomial"""
    out = np.zeros((2, len(q), n), dtype=np.uint64)
    out[0, :, 0] = np.array([c % p for p in q], dtype=np.uint64)
    return out


def _y_cases(sc, which, rnd):
    cases = []
    for i, p in enumerate(sc.q):
        for nm, val in y_points(p).items():
            tgt = [rnd.randrange(x) for x in sc.q]
            tgt[i] = val
            cases.append(("%s.y%d=%s" % (which, i, nm), sc.y_for(tgt, which)))
    cases.append(("%s.all=m-1" % which, sc.y_for([p - 1 for p in sc.q], which)))
    cases.append(("%s.all=0" % which, [0] * sc.k))
    return cases


def lift_cases(q, n, seed=1):
    """steps 0/1: every y_i at each of y_points (the others random), all y_i at q_i - 1 (the largest column sum), all at 0, and
    the centred remainder r at each of R_TARGETS -- the other y_i held at q_i - 1 - 2^33, the low word of the last y solved
    (punct_q_mod_mt of the last prime is odd) -- and, for k >= 2, r = 0x80000000 together with y_0 = 0"""
    sc, rnd = Scalar(q, 2, seal_aux(q)), random.Random(seed)               # the lift does not involve t or the auxiliary base
    cases = _y_cases(sc, "lift", rnd)
    q_mt, base = sc.Q & M32, len(cases)
    inv_last = pow(sc.punct_mod_mt[-1], -1, MT)
    for r in R_TARGETS + ((0x80000000,) if sc.k > 1 else ()):             # the seventh: the boundary once more, with y_0 = 0
        y = [p - 1 - (1 << 33) for p in sc.q]
        if len(cases) >= base + len(R_TARGETS):
            y[0] = 0
        others = sum((v & M32) * m for v, m in zip(y[:-1], sc.punct_mod_mt[:-1]))
        low = ((-r * q_mt - others) * inv_last) & M32                      # r = -x q^-1  <=>  x = -r q  (mod 2^32)
        y[-1] = (y[-1] >> 32 << 32) | low
        cases.append(("lift.y0=0&r=0x80000000" if y[0] == 0 else "lift.r=0x%08X" % r, sc.y_for(y, "lift")))
    return _place(q, n, cases, seed)


def floor_y_cases(q, t, n, seed=2):
    """step 3 with the other operand (1, 0): D = lift(a) = a (mod q), so a_i = y_i (t (q/q_i)^-1)^-1 gives any y_i"""
    sc, rnd = Scalar(q, t, seal_aux(q)), random.Random(seed)
    cases = _y_cases(sc, "floor", rnd)
    for sign in (">=0", "<0"):                                             # both signs of v among plain random coefficients too
        while True:
            a = [rnd.randrange(p) for p in q]
            if (sc.coefficient(a, 1)[1]["v"] >= 0) == (sign == ">=0"):
                cases.append(("floor.v" + sign, a))
                break
    return _place(q, n, cases, seed)


def floor_z_cases(q, t, aux, n, seed=3, max_tries=4000):
    """step 4 with the other operand (c, 0), c = floor_constant: for each of floor_z_targets(shared=True) take its floor value v*
    and draw a' from [v* q / (t c), (v* + k) q / (t c)] until the model gives v == v* with lift(a' mod q) == a'.
    Returns (operand, labels, c, the largest number of model evaluations one target took)."""
    sc, rnd = Scalar(q, t, aux), random.Random(seed)
    c = floor_constant(q, t, aux)
    assert c < sc.Q // 4
    cases, worst = [], 0
    for label in floor_z_targets(q, t, aux, shared=True):
        vstar = _parse_z(sc, label)
        lo, hi = vstar * sc.Q // (t * c), (vstar + sc.k) * sc.Q // (t * c)
        for tries in range(1, max_tries + 1):
            ap = rnd.randrange(lo, hi + 1)
            a = [ap % p for p in q]
            lf, fl = sc.coefficient(a, c)
            if fl["v"] == vstar and lf["value"] == ap:
                break
        else:
            raise AssertionError("no operand found for " + label)
        worst = max(worst, tries)
        cases.append((label, a))
    a, labels = _place(q, n, cases, seed)
    return a, labels, c, worst


def floor_z_extra_cases(q, t, aux, n, seed=4, max_tries=20000):
    """the targets outside the shared sweep (floor_z_targets(shared=False): |v*| near b_j on a q too short for t 2^s >= 4 b_j), each
    against a constant of its own that is no power of two: draw c from [q / 8, q / 4) and take a' next to v* q / (t c) -- a fraction q / (t a') ~ 2^-8 of
    the draws has t a' c land in the one window of width q that gives v == v* -- with lift(a' mod q) == a' and lift(c) == c.
    Returns [(operand, labels, c)], one per target, and the largest number of model evaluations one target took."""
    sc, rnd = Scalar(q, t, aux), random.Random(seed)
    out, worst = [], 0
    for idx, label in enumerate(floor_z_targets(q, t, aux, shared=False)):
        vstar = _parse_z(sc, label)
        for tries in range(1, max_tries + 1):
            c = rnd.randrange(sc.Q // 8, sc.Q // 4)
            ap = -((-(vstar + rnd.randrange(sc.k)) * sc.Q) // (t * c))           # ceil
            a = [ap % p for p in q]
            lf, fl = sc.coefficient(a, c)
            if fl["v"] == vstar and lf["value"] == ap and abs(ap) < sc.Q // 4 and sc.lift([c % p for p in q])["value"] == c:
                break
        else:
            raise AssertionError("no operand found for " + label)
        worst = max(worst, tries)
        out.append(_place(q, n, [(label, a)], seed + idx) + (c,))
    return out, worst


def magnitude_cases(q, n, size):
    """operands of maximal centred magnitude: every coefficient of every polynomial is floor(q/2) (first operand) or ceil(q/2)
    (second).  Returns (lo [size][k][n], hi [size][k][n])."""
    H = prod(q) // 2
    lo = np.empty((size, len(q), n), dtype=np.uint64)
    hi = np.empty_like(lo)
    for i, p in enumerate(q):
        lo[:, i, :] = H % p
        hi[:, i, :] = (H + 1) % p
    return lo, hi


def magnitude_D(la, lb, sa, sb, n):
    """the tensor sums of operands whose lifts are the constants la and lb in every coefficient: the negacyclic product of two
    all-ones polynomials has coefficient 2 j + 2 - n at x^j, and output polynomial o has min(o, sa - 1, sb - 1, sa + sb - 2 - o) + 1 terms"""
    so = sa + sb - 1
    return [[(min(o, sa - 1, sb - 1, so - 1 - o) + 1) * la * lb * (2 * j + 2 - n) for j in range(n)] for o in range(so)]
