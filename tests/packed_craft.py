"""The packed integer maps (csrc/packed.hip: k_block8x8, k_channel_mix; csrc/planemap.hip: pm_output; csrc/packed_arith.h) restated in
integers, and the operands that drive them to their arithmetic edges.  Nothing here calls the library.

The model.  numpy uint64 wraps modulo 2^64 exactly as the device words do.  mul_lazy4 is mul_shoup_lazy4: the low 64 bits of
x w + A (2^64 - q) with A the truncated high word of x w' as coded (hi(xh pl) + hi(xl ph) + xh ph: the low x low partial product and the
carries of the cross terms are left out).  Its value is x w mod q + e q; e = y div q is the EXCESS of the product.  mul_shoup is the exact
Shoup product with one conditional subtraction.  block_model, mix_model and pm_model follow the kernels' order of operations and return
the output words and a trace: every unreduced sum, the excess of every product, the value entering canon().  The maps are element-wise in
(polynomial, prime, coefficient): an array [planes, k, P] holds P = size n independent instances per prime ("positions"; position
s n + j is coefficient j of polynomial s, to_ct / to_pos change between the two layouts).

The reach table (reach_excess): per prime and product site the largest excess a seeded search finds with the operand anywhere below the
site's documented bound -- 2^18 products per site and prime, 256 weights (both ends of the range, +-1, half of them negative) by 1024
operands.  DESIGN.md 3.12.1 records it; tests/test_packed_craft_cpu.py asserts it and counts, in the traces, what the families reach.

The families.  Every position has ONE target (`tgt`, in rotation over the positions); its input residues are solved or searched for it:
  S   lazy sums: all eight terms of one sum at a prescribed excess with residues in the top sixteenth of [0, q); in plane map also a
      64-term output whose eight chunk sums are multiples of q, so that every chunk value carries the excess 1 of its product by 1
  X   exits: the value entering canon() in each interval [j q, (j + 1) q) the table allows; the final residue exactly 0 and exactly
      q - 1, each in the highest interval the exit's product can return for it (exit_hi tries every operand that gives the residue: 0
      always leaves the product with an excess of at least 1, q - 1 never with the Shoup quotient's own error); the last input is
      solved for the residue and the others are drawn again, the draw in the highest interval kept
  C   canonical sums: the inputs solved so that all eight products of one sum are q - 1 (8 q - 8 unreduced), outputs exactly 0 and q - 1
All inputs are canonical residues; all weights obey |w| <= min((t - 1) / 2, 2^31 - 1) and hold both ends of that range; the rows of L, R
and M a target is aimed at are dense and negative (a positive weight below 2^31 has a Shoup companion below 2^32 at these primes, which
leaves two of the three truncated partial products out and caps the excess at 1)."""
import numpy as np

import galois_oracle as go
import packed_oracle as po
from test_gpu_galois import _is_prime, _primes_58
from test_gpu_packed import _prime_61

U = np.uint64
M32, S32 = U(0xFFFFFFFF), U(32)
N = 1024
SEED = 20263
NOPM = {"FHE_NTT_NOPM": "1"}
T_SMALL = 65537                                                  # (t - 1) / 2 = 32768 is the scalar limit there
WITNESS = (0x3FFFFFFFFFF9001, 0x78B2B578C230FCE6, -474698375)      # q, x, w: mul_shoup_lazy4 returns 3 q + (x w mod q)
ROUNDS = 256                                                     # the budget of every re-draw loop
CANDIDATES = 96                                                  # candidates per term of a family-S sum
HEAVY = 48                                                       # positions of a target that needs 32 times the candidates


def prime_below(bits, n=N):
    """the largest prime below 2^bits that is 1 (mod 2n)"""
    m = (1 << bits) + 1
    while True:
        m -= 2 * n
        if _is_prime(m):
            return m


def bases():
    """name -> (primes, switches), all at n = 1024"""
    return {"Q3": (list(go.Q3), {}), "Q4": (list(go.Q4), {}), "Q58": (_primes_58(N, 2), {}), "shoup": (list(go.Q4), dict(NOPM)),
            "Q60": ([prime_below(60), go.Q4[0]], {}), "Q61": ([_prime_61(N), go.Q4[0]], {})}


def gate(q, switches=None):
    """lazy_ok (packed_arith.h): the lazy sums run when the widest prime has at most 58 bits and FHE_NTT_NOPM is not set"""
    return max(int(p).bit_length() for p in q) <= 58 and not (switches or {}).get("FHE_NTT_NOPM")


# ---- the arithmetic ------------------------------------------------------------------------------------------------------------------
def lift_pair(w, q):
    a = abs(int(w)) % q
    r = q - a if (w < 0 and a) else a
    return r, (r << 64) // q


def pairs(W, q):
    """(w mod q_i, Shoup companion) of integer weights W [...]: two uint64 arrays [..., k, 1]; a zero weight is the pair (0, 0)"""
    W = np.asarray(W, dtype=np.int64)
    w, wp = np.zeros(W.shape + (len(q), 1), dtype=U), np.zeros(W.shape + (len(q), 1), dtype=U)
    for idx in np.ndindex(W.shape):
        for i, qi in enumerate(q):
            w[idx + (i, 0)], wp[idx + (i, 0)] = lift_pair(W[idx], int(qi))
    return w, wp


def hi64(x, p):
    """__umul64hi, exact"""
    xl, xh, pl, ph = x & M32, x >> S32, p & M32, p >> S32
    lh, hl = xl * ph, xh * pl
    mid = ((xl * pl) >> S32) + (lh & M32) + (hl & M32)
    return xh * ph + (lh >> S32) + (hl >> S32) + (mid >> S32)


def hi64_lazy4(x, p):
    """the high word mul_shoup_lazy4 takes: s = hi(xh pl) + hi(xl ph) with its carry, A = xh ph + (cy : s)"""
    xl, xh, pl, ph = x & M32, x >> S32, p & M32, p >> S32
    return xh * ph + (((xh * pl) >> S32) + ((xl * ph) >> S32))


def mul_lazy4(x, w, wp, q):
    """mul_shoup_lazy4: (hi : lo) of P = al nl + xl wl and C = ah nl + al nh + xh wl + xl wh is the low 64 bits of x w + A (2^64 - q)"""
    return x * w + hi64_lazy4(x, wp) * (U(0) - q)


def mul_shoup(x, w, wp, q):
    r = x * w - hi64(x, wp) * q
    return np.where(r >= q, r - q, r)


class Arith:
    """PkArith<LAZY> over the primes q (arrays [..., k, P]); canon_once: the variant whose canon() subtracts q once"""

    def __init__(self, q, lazy, canon_once=False):
        self.q, self.lazy, self.canon_once = [int(p) for p in q], bool(lazy), canon_once
        self.qa = np.array(self.q, dtype=U)[:, None]
        self.one = pairs(1, self.q)

    def mul(self, x, pr):
        return mul_lazy4(x, pr[0], pr[1], self.qa) if self.lazy else mul_shoup(x, pr[0], pr[1], self.qa)

    def canon(self, y):
        if not self.lazy:
            return y
        if not self.canon_once:
            y = np.where(y >= U(2) * self.qa, y - U(2) * self.qa, y)
        return np.where(y >= self.qa, y - self.qa, y)

    def e(self, y):
        """the excess of a product; a canonical product has none"""
        return (y // self.qa).astype(np.uint8) if self.lazy else np.zeros(y.shape, dtype=np.uint8)

    def units(self, s):
        """an unreduced sum in units of q, rounded down"""
        return s // self.qa


def to_pos(ct):
    """[planes, size, k, n] -> [planes, k, size n]"""
    p, s, k, n = ct.shape
    return np.ascontiguousarray(ct.transpose(0, 2, 1, 3)).reshape(p, k, s * n)


def to_ct(pos, size):
    p, k, sn = pos.shape
    return np.ascontiguousarray(pos.reshape(p, k, size, sn // size).transpose(0, 2, 1, 3))


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------
def block_tab(q, L, R, pre=None, post=None):
    """B8Tab: pre is absent for a plan without one (k_block8x8<*, false>); post is the pair for 1 then"""
    sq = lambda a: np.asarray(a, dtype=np.int64).reshape(8, 8)
    return dict(pre=None if pre is None else pairs(sq(pre), q), L=pairs(sq(L), q), R=pairs(sq(R), q),
                post=pairs(np.ones((8, 8), dtype=np.int64) if post is None else sq(post), q))


def block_model(A, X, tab):
    """k_block8x8<LAZY, PRE>: X [64, k, P] -> (out [64, k, P], trace).  pre; the eight row lines mid[x][v] = sum_y r[x][y] R[v][y]; the eight
    column lines o[u][v] = sum_x mid[x][v] L[u][x]; post (or 1); canon.  row_e [x][v][y], col_e [u][v][x]."""
    k, P = X.shape[-2:]
    r, tr = X.reshape(8, 8, k, P), {}
    if tab["pre"] is not None:
        r = A.mul(r, tab["pre"])
        tr["pre_e"] = A.e(r)
    (Rw, Rp), (Lw, Lp) = tab["R"], tab["L"]
    mid, o = np.empty((8, 8, k, P), dtype=U), np.empty((8, 8, k, P), dtype=U)
    row_e, col_e = np.empty((8, 8, 8, k, P), dtype=np.uint8), np.empty((8, 8, 8, k, P), dtype=np.uint8)
    for v in range(8):
        t = A.mul(r, (Rw[v][None], Rp[v][None]))                       # [x][y]
        mid[:, v], row_e[:, v] = t.sum(axis=1, dtype=U), A.e(t)
    for u in range(8):
        t = A.mul(mid, (Lw[u][:, None], Lp[u][:, None]))               # [x][v]
        o[u], col_e[u] = t.sum(axis=0, dtype=U), np.moveaxis(A.e(t), 0, 1)
    y = A.mul(o, tab["post"])
    tr.update(mid=mid, row_e=row_e, o=o, col_e=col_e, post_e=A.e(y), canon_in=y)
    return A.canon(y).reshape(64, k, P), tr


def block_chain(A, X, tab, u, v):
    """the value entering canon() at output (u, v) alone"""
    k, P = X.shape[-2:]
    r = X.reshape(8, 8, k, P)
    if tab["pre"] is not None:
        r = A.mul(r, tab["pre"])
    mid = A.mul(r, (tab["R"][0][v][None], tab["R"][1][v][None])).sum(axis=1, dtype=U)
    o = A.mul(mid, (tab["L"][0][u], tab["L"][1][u])).sum(axis=0, dtype=U)
    return A.mul(o, (tab["post"][0][u, v], tab["post"][1][u, v]))


def mix_model(A, V, Mp, extra_term=False):
    """k_channel_mix<LAZY>: V [c, k, P], Mp = pairs(M [m][c]) -> out [m, k, P]; extra_term: the variant that adds a ninth term (the first, again)"""
    t = A.mul(V[None], Mp)
    acc = t.sum(axis=1, dtype=U)
    if extra_term:
        acc = acc + t[:, 0]
    y = A.mul(acc, A.one)
    return A.canon(y), dict(term_e=A.e(t), terms=t, acc=acc, one_e=A.e(y), canon_in=y)


def pm_tab(q, taps, weights):
    """the plan's term lists: per output the live (tap, weight) in slot order, padded to a multiple of four with (first tap, pair (0, 0))"""
    out = []
    for trow, wrow in zip(np.asarray(taps), np.asarray(weights)):
        live = np.nonzero(wrow)[0]
        tp, wt = [int(trow[j]) for j in live], [int(wrow[j]) for j in live]
        while len(tp) % 4:
            tp.append(tp[0])
            wt.append(0)
        out.append((np.array(tp), pairs(wt, q), len(live)))
    return out


def pm_model(A, planes, tab, chunk=8, reduce_chunks=True):
    """pm_output<LAZY> for every output: planes [n_in, k, P] -> (out [n_out, k, P], one trace per output).  Chunks of two quads; with more
    than two quads every chunk goes through the product by 1; the total through the product by 1 and canon.  chunk = 16 and
    reduce_chunks = False are the wrong variants."""
    outs, traces = [], []
    for tp, pr, _ in tab:
        t = A.mul(planes[tp], pr)
        n_quads, nc = len(tp) // 4, -(-len(tp) // chunk)
        full = np.zeros((nc * chunk,) + t.shape[1:], dtype=U)
        full[:len(tp)] = t
        acc = full.reshape((nc, chunk) + t.shape[1:]).sum(axis=1, dtype=U)
        multi = n_quads > chunk // 4
        cv = A.mul(acc, A.one) if (multi and reduce_chunks) else acc
        total = cv.sum(axis=0, dtype=U)
        y = A.mul(total, A.one)
        outs.append(A.canon(y))
        traces.append(dict(term_e=A.e(t), terms=t, acc=acc, chunk_e=A.e(cv) if (multi and reduce_chunks) else None, cv=cv, total=total, one_e=A.e(y), canon_in=y, multi=multi))
    return np.stack(outs), traces


# ---- the reach table -----------------------------------------------------------------------------------------------------------------
# site -> the operand's documented bound in units of q.  "row" is the row term of a plan without pre (a canonical operand), "row_pre"
# the one behind a pre product; the products by 1 are k_block8x8's in a plan without post, channel_mix's, plane_map's per chunk and
# plane_map's on the total.
SITES = {"pre": 1, "row": 1, "row_pre": 4, "col": 32, "post": 32, "one_block": 32, "one_mix": 32, "one_chunk": 32, "one_total": 32}
_reach = {}


def reach_weights(rng, lim, count=256):
    w = rng.integers(1, lim + 1, size=count, dtype=np.int64)
    w[::2] *= -1
    w[:4] = (-lim, lim, -1, 1)
    return w


def reach_excess(q, t=po.T33, seed=SEED, operands=1024):
    """per site the largest excess per prime of q: 256 weights x `operands` operands uniform below the site's bound (one weight, 1, and
    256 x `operands` operands for the products by 1).  Lazy arithmetic whatever the primes' width: below 2^64 / 32 nothing wraps."""
    key = (tuple(q), t, seed, operands)
    if key not in _reach:
        A = Arith(q, True)
        rng = np.random.default_rng(seed)
        W = reach_weights(rng, po.scalar_limit(t))
        pw = pairs(W, q)
        out = {}
        with np.errstate(over="ignore"):
            for site, bound in SITES.items():
                x = rng.integers(0, U(bound) * A.qa, size=(W.size, len(q), operands), dtype=U)
                y = A.mul(x, (A.one[0][None], A.one[1][None]) if site.startswith("one") else pw)
                out[site] = [int(v) for v in A.e(y).max(axis=(0, 2))]
        _reach[key] = out
    return _reach[key]


def witness():
    """the excess of WITNESS, the operand and weight the comment of mul_shoup_lazy4 (csrc/modarith.h) cites: found by a random search
    over negative weights and operands from 8 q on at the largest 58-bit prime"""
    q, x, w = WITNESS
    A = Arith([q], True)
    y = int(A.mul(np.array([[x]], dtype=U), pairs(w, [q]))[0, 0])
    r, _ = lift_pair(w, q)
    assert y % q == x * r % q
    return y // q


# ---- helpers of the builders ---------------------------------------------------------------------------------------------------------
def _inv(a, q):
    return pow(int(a) % q, -1, q)


def _top16(rng, A, shape):
    """residues in the top sixteenth of [0, q)"""
    w = A.qa // U(16)
    return (A.qa - w) + rng.integers(0, w, size=shape, dtype=U)


def _uniform(rng, A, shape):
    return rng.integers(0, A.qa, size=shape, dtype=U)


def _pick(cands, score, want):
    """cands [C, ..., k, P], score [C, k, P], want [k, 1]: per (prime, position) the first candidate whose score is `want` (else the first)"""
    idx = (score == want[None]).argmax(axis=0)
    extra = cands.ndim - 3
    ix = np.broadcast_to(idx.reshape((1,) + (1,) * extra + idx.shape), (1,) + cands.shape[1:])
    return np.take_along_axis(cands, ix, axis=0)[0]


def _mulmod_rows(a, consts, q):
    """a [k, P] times one constant per prime, modulo each prime"""
    return np.stack([po.mulmod(a[i], int(consts[i]) % int(q[i]), int(q[i])) for i in range(len(q))])


def _weights(rng, lim, shape, negative=False):
    w = rng.integers(1, lim + 1, size=shape, dtype=np.int64)
    if not negative:
        w *= rng.choice(np.array([-1, 1]), size=shape)
    return -w if negative else w


def _aimed(rng, A, lim, count, lo, hi, level, pool=512):
    """`count` negative weights for the terms of a targeted sum.  How often a product has a given excess depends on the weight (-(2^31 - 1)
    never gives 2 on a canonical operand of the 58-bit primes; one weight in eight gives 3 at all): of a seeded pool the `count` weights
    whose excess is `level` [k, 1] most often, on the rarest prime, over operands uniform in [lo q, hi q) are kept (lo, hi in sixteenths)."""
    lo, hi = int(lo * 16), int(hi * 16)
    with np.errstate(over="ignore"):
        x = U(lo) * (A.qa // U(16)) + rng.integers(0, U(hi - lo) * (A.qa // U(16)), size=(len(A.q), 4096 if int(level.max()) == 3 else 1024), dtype=U)
        cand = -rng.integers(1, lim + 1, size=pool, dtype=np.int64)
        rate = (A.e(A.mul(x[None], pairs(cand, A.q))) == level[None]).mean(axis=2).min(axis=1)
    return cand[np.argsort(-rate, kind="stable")[:count]]


def _rotation(P, names, fixed=None):
    tgt = np.arange(P) % len(names)
    for p, name in (fixed or {}).items():
        tgt[p] = names.index(name)
    return tgt


def _frozen(emax):
    """a hashable form of a reach table's rows (None: the table of reach_excess)"""
    return None if emax is None else tuple(sorted((s_, tuple(v)) for s_, v in emax.items()))


class Case(dict):
    __getattr__ = dict.__getitem__


def _levels(emax):
    """the family-S levels per prime: 2 (or the site's largest excess where that is smaller) and, where it is reachable, 3"""
    e = np.array(emax, dtype=np.uint8)[:, None]
    return {"e2": np.minimum(e, 2), "e3": e} if (e == 3).any() else {"e2": np.minimum(e, 2)}


def _redraw(A, P_sel, draw, value, want, rounds=ROUNDS):
    """the re-draw loop of family X: draw() gives inputs [planes, k, P'], value(X) the word entering canon() [k, P']; keeps, per (prime,
    position), the first draw whose interval is want [k, 1]; the last draw where none fits within `rounds`"""
    X = draw(P_sel)
    done = A.units(value(X)) == want
    for _ in range(rounds):
        if done.all():
            break
        Y = draw(P_sel)
        ok = (A.units(value(Y)) == want) & ~done
        X = np.where(ok[None], Y, X)
        done |= ok
    return X


def _redraw_max(A, P_sel, draw, value, rounds=ROUNDS):
    """the re-draw loop of the residue targets: of `rounds` draws the one whose word entering canon() lies in the highest interval, per
    (prime, position)"""
    X = draw(P_sel)
    best = A.units(value(X))
    for _ in range(rounds):
        Y = draw(P_sel)
        iv = A.units(value(Y))
        X = np.where((iv > best)[None], Y, X)
        best = np.maximum(best, iv)
    return X


def exit_hi(A, pair, residue, terms=32):
    """the highest interval the last product can return with the final residue 0 (residue = 0) or q - 1 (1), per prime [k, 1]: its
    operand is then one of the `terms` values x0 + j q below `terms` q, x0 = residue / w mod q -- all of them are tried"""
    xs = np.empty((len(A.q), terms), dtype=U)
    for i, p in enumerate(A.q):
        x0 = (p - 1 if residue else 0) * _inv(pair[0][i, 0], p) % p
        xs[i] = [x0 + j * p for j in range(terms)]
    with np.errstate(over="ignore"):
        return A.units(A.mul(xs, pair)).max(axis=1)[:, None] if A.lazy else np.zeros((len(A.q), 1), dtype=U)


# ---- fhe_block8x8_scalar -------------------------------------------------------------------------------------------------------------
X0, V0, U0 = 2, 5, 3                      # the row line (X0, V0) and the output (U0, V0) the targets are aimed at; the last input (7, 7) is the solved one
_cases = {}


def block_plan(A, t, pre, post, emax, seed=SEED, aim=True):
    """dense L and R with both ends of the range in rows no target uses; row V0 of R, row U0 of L, row X0 of pre and post[U0][V0] are the
    aimed weights (_aimed) of their sites"""
    rng = np.random.default_rng(seed + 2 * pre + post)
    lim = po.scalar_limit(t)
    lv = lambda site, cap: np.minimum(np.array(emax[site], dtype=np.uint8)[:, None], cap)
    L, R = _weights(rng, lim, (8, 8)), _weights(rng, lim, (8, 8))
    choose = _aimed if aim else (lambda rng, A, lim, count, *a: _weights(rng, lim, count, True))
    R[V0] = choose(rng, A, lim, 8, 0, 4, lv("row_pre", 2)) if pre else choose(rng, A, lim, 8, 15 / 16, 1, lv("row", 2))
    L[U0] = choose(rng, A, lim, 8, 16, 20, lv("col", 3))
    L[0, 0], L[7, 7], R[0, 7], R[7, 0] = lim, -lim, -lim, lim
    p0 = p1 = None
    if pre:
        p0 = _weights(rng, lim, (8, 8))
        p0[X0] = _weights(rng, lim, 8, True)
        p0[0, 0], p0[7, 6] = lim, -lim
    if post:
        p1 = _weights(rng, lim, (8, 8))
        p1[0, 0], p1[7, 7] = lim, -lim
        p1[U0, V0] = choose(rng, A, lim, 1, 16, 20, lv("post", 3))[0]
    return L, R, p0, p1


def _coef(q, L, R, pre, post, u, v, x, y):
    """the coefficient of input (x, y) in output (u, v), per prime"""
    return [int(L[u][x]) * int(R[v][y]) * (1 if pre is None else int(pre[x][y])) * (1 if post is None else int(post[u][v])) % int(p) for p in q]


def _matinv(M, q):
    """the inverse of an 8x8 integer matrix modulo the prime q (Gauss-Jordan on Python integers); None when it is singular"""
    n = len(M)
    a = [[int(M[i][j]) % q for j in range(n)] + [int(i == j) for j in range(n)] for i in range(n)]
    for c in range(n):
        piv = next((r for r in range(c, n) if a[r][c]), None)
        if piv is None:
            return None
        a[c], a[piv] = a[piv], a[c]
        inv = pow(a[c][c], -1, q)
        a[c] = [v * inv % q for v in a[c]]
        for r in range(n):
            if r != c and a[r][c]:
                f = a[r][c]
                a[r] = [(vr - f * vc) % q for vr, vc in zip(a[r], a[c])]
    return [row[n:] for row in a]


def craft_block(q, lazy, pre, post, size=2, t=po.T33, seed=SEED, emax=None):
    """one group of 64 ciphertexts: Case(X [64, k, P], tgt, names, plan, tab, A).  `lazy` chooses the families (S and X, or C), whatever
    the primes' width (the wrong-gate variants run family S at 60 and 61 bits); emax: the reach table's rows, reach_excess(q, t) by default."""
    key = ("block", tuple(q), lazy, pre, post, size, t, seed, _frozen(emax))
    if key in _cases:
        return _cases[key]
    A = Arith(q, lazy)
    rng = np.random.default_rng(seed + 17 * pre + 31 * post + size)
    emax = emax or (reach_excess(q, t) if lazy else {s_: [2] * len(q) for s_ in SITES})
    L, R, p0, p1 = block_plan(Arith(q, True), t, pre, post, emax, seed, aim=lazy)
    tab = block_tab(q, L, R, p0, p1)
    k, P = len(q), size * N
    pick_tab = lambda name, a, b: (tab[name][0][a, b], tab[name][1][a, b])
    with np.errstate(over="ignore"):
        if lazy:
            row_lv, col_lv = _levels(emax["row_pre" if pre else "row"]), _levels(emax["col"])
            top = np.array(emax["post" if post else "one_block"], dtype=U)[:, None]
            names = ["S_row_" + n for n in row_lv] + ["S_col_" + n for n in col_lv] + ["X_%d" % j for j in range(int(top.max()) + 1)] + ["X_hi_0", "X_hi_qm1", "random"]
            tgt = _rotation(P, names)
            X = _top16(rng, A, (64, k, P))
            X[:, :, tgt == names.index("random")] = _uniform(rng, A, (64, k, int((tgt == names.index("random")).sum())))
            for n, lv in row_lv.items():                               # S: row line (X0, V0), term by term
                sel = tgt == names.index("S_row_" + n)
                for y in range(8):
                    c = _top16(rng, A, (CANDIDATES, k, int(sel.sum())))
                    r = A.mul(c, pick_tab("pre", X0, y)) if pre else c
                    X[8 * X0 + y][:, sel] = _pick(c, A.e(A.mul(r, pick_tab("R", V0, y))), lv)
            for n, lv in col_lv.items():                               # S: column line (U0, V0); term x depends on input row x alone
                sel = tgt == names.index("S_col_" + n)
                if n == "e3":                                          # rare (one product in a few hundred, and only from about 20 q on): HEAVY positions
                    sel &= np.cumsum(sel) <= HEAVY
                for x in range(8):
                    c = _top16(rng, A, (CANDIDATES, 8, k, int(sel.sum())))
                    r = A.mul(c, (tab["pre"][0][x][None], tab["pre"][1][x][None])) if pre else c
                    if n == "e3":                                      # 32 times the candidates, each put together from inputs whose row terms have excess 2
                        good = A.e(A.mul(r, (tab["R"][0][V0][None], tab["R"][1][V0][None]))) == 2
                        first = np.argsort(-(good + 0.5 * rng.random(good.shape)), axis=0)
                        ix = rng.integers(0, 1 << 31, size=(32 * CANDIDATES,) + good.shape[1:]) % np.maximum(good.sum(axis=0), 1)[None]
                        c = np.take_along_axis(c, np.take_along_axis(first, ix, axis=0), axis=0)
                        r = A.mul(c, (tab["pre"][0][x][None], tab["pre"][1][x][None])) if pre else c
                    mid = A.mul(r, (tab["R"][0][V0][None], tab["R"][1][V0][None])).sum(axis=1, dtype=U)
                    X[8 * x:8 * x + 8][:, :, sel] = _pick(c, A.e(A.mul(mid, pick_tab("L", U0, x))), lv)
            cinv = [_inv(c, p) for c, p in zip(_coef(q, L, R, p0, p1, U0, V0, 7, 7), q)]
            value = lambda Z: block_chain(A, Z, tab, U0, V0)

            def solved(residue):
                def draw(n):
                    Z = _top16(rng, A, (64, k, n))
                    have = A.canon(value(Z))
                    want = np.broadcast_to(np.array([p - 1 if residue else 0 for p in A.q], dtype=U)[:, None], have.shape)
                    d = _mulmod_rows((want + (A.qa - have)) % A.qa, cinv, A.q)
                    Z[63] = (Z[63] + d) % A.qa
                    return Z
                return draw
            for j in range(int(top.max()) + 1):
                sel = tgt == names.index("X_%d" % j)
                X[:, :, sel] = _redraw(A, int(sel.sum()), lambda n: _top16(rng, A, (64, k, n)), value, np.minimum(top, U(j)))
            for name, residue in (("X_hi_0", 0), ("X_hi_qm1", 1)):
                sel = tgt == names.index(name)
                X[:, :, sel] = _redraw_max(A, int(sel.sum()), solved(residue), value, 64)
        else:
            names = ["C_row", "C_col", "C_0", "C_qm1", "random"]
            tgt = _rotation(P, names)
            X = _uniform(rng, A, (64, k, P))
            pre_ = np.ones((8, 8), dtype=np.int64) if p0 is None else p0
            for i, p in enumerate(A.q):
                # C_row: every product of the eight row lines (x, V0) is q - 1: pre[x][y] X[x][y] R[V0][y] = -1
                sol = np.array([[(p - 1) * _inv(int(R[V0][y]) * int(pre_[x][y]), p) % p for y in range(8)] for x in range(8)], dtype=U).reshape(64)
                X[:, i, tgt == 0] = sol[:, None]
                # C_col: every product of the column lines (U0, v) is q - 1: mid[x][v] = -1 / L[U0][x] for all v, so R (pre[x] . X[x]) = that vector
                Rinv = _matinv(R, p)
                assert Rinv is not None, "R is singular modulo a prime: another seed"
                for x in range(8):
                    m = (p - 1) * _inv(L[U0][x], p) % p
                    z = [sum(Rinv[y][v] for v in range(8)) * m % p for y in range(8)]
                    X[8 * x:8 * x + 8, i, tgt == 1] = np.array([z[y] * _inv(pre_[x][y], p) % p for y in range(8)], dtype=U)[:, None]
            cinv = [_inv(c, p) for c, p in zip(_coef(q, L, R, p0, p1, U0, V0, 7, 7), q)]
            for name, residue in (("C_0", 0), ("C_qm1", 1)):
                sel = tgt == names.index(name)
                Z = X[:, :, sel]
                have = block_chain(A, Z, tab, U0, V0)
                want = np.broadcast_to(np.array([p - 1 if residue else 0 for p in A.q], dtype=U)[:, None], have.shape)
                Z[63] = (Z[63] + _mulmod_rows((want + (A.qa - have)) % A.qa, cinv, A.q)) % A.qa
                X[:, :, sel] = Z
    _cases[key] = Case(X=X, tgt=tgt, names=names, plan=(L, R, p0, p1), tab=tab, A=A, size=size, emax=emax)
    return _cases[key]


def count_block(case, tr, out):
    """name -> positions per prime at which the trace meets the target (wherever it does, whatever the position was aimed at)"""
    A, X = case.A, case.X
    hi = X >= A.qa - A.qa // U(16)
    res = {}
    if A.lazy:
        e = case.emax
        for n, lv in _levels(e["row_pre" if case.plan[2] is not None else "row"]).items():
            res["S_row_" + n] = ((tr["row_e"][X0, V0] == lv[None]).all(axis=0) & hi[8 * X0:8 * X0 + 8].all(axis=0)).sum(axis=1)
        for n, lv in _levels(e["col"]).items():
            res["S_col_" + n] = ((tr["col_e"][U0, V0] == lv[None]).all(axis=0) & hi.all(axis=0)).sum(axis=1)
        if case.plan[2] is not None:                                  # the pre site: some pre product of the position at the site's largest excess
            res["site_pre"] = (tr["pre_e"] == np.array(e["pre"], dtype=np.uint8)[:, None]).any(axis=(0, 1)).sum(axis=1)
        iv = A.units(tr["canon_in"][U0, V0])
        top = np.array(e["post" if case.plan[3] is not None else "one_block"], dtype=U)[:, None]
        o = out.reshape(8, 8, *out.shape[1:])[U0, V0]
        for j in range(int(top.max()) + 1):
            res["X_%d" % j] = np.where(top[:, 0] >= j, (iv == U(j)).sum(axis=1), -1)          # -1: not reachable at that prime
        ex = (case.tab["post"][0][U0, V0], case.tab["post"][1][U0, V0])
        res["X_hi_0"] = ((iv == exit_hi(A, ex, 0)) & (o == 0)).sum(axis=1)
        res["X_hi_qm1"] = ((iv == exit_hi(A, ex, 1)) & (o == A.qa - U(1))).sum(axis=1)
    else:
        qm1 = A.qa - U(1)
        res["C_row"] = (tr["mid"][:, V0] == U(8) * qm1).all(axis=0).sum(axis=1)
        res["C_col"] = (tr["o"][U0] == U(8) * qm1).all(axis=0).sum(axis=1)
        o = out.reshape(8, 8, *out.shape[1:])[U0, V0]
        res["C_0"], res["C_qm1"] = (o == 0).sum(axis=1), (o == qm1).sum(axis=1)
    return {n: [int(v) for v in c] for n, c in res.items()}


# ---- fhe_channel_mix -----------------------------------------------------------------------------------------------------------------
O0 = 1                                    # the output row the targets are aimed at (0 for m = 1); input 7 is the solved one


def mix_plan(A, t, m, emax, seed=SEED, aim=True):
    rng = np.random.default_rng(seed + m)
    lim = po.scalar_limit(t)
    M = _weights(rng, lim, (m, 8))
    M[0, 0], M[m - 1, 7] = lim, -lim
    M[O0] = _aimed(rng, A, lim, 8, 15 / 16, 1, np.minimum(np.array(emax["row"], dtype=np.uint8)[:, None], 2)) if aim else _weights(rng, lim, 8, True)
    return M


def craft_mix(q, lazy, m, size=2, t=po.T33, seed=SEED, emax=None):
    """c = 8 planes of one ciphertext: Case(X [8, k, P], ...).  Position 0 (coefficient 0 of c0) is aimed at output O0 = q - 1, so that a
    bias on that output wraps past q there."""
    key = ("mix", tuple(q), lazy, m, size, t, seed, _frozen(emax))
    if key in _cases:
        return _cases[key]
    A = Arith(q, lazy)
    rng = np.random.default_rng(seed + 5 * m + size)
    emax = emax or (reach_excess(q, t) if lazy else {s_: [2] * len(q) for s_ in SITES})
    M = mix_plan(Arith(q, True), t, m, emax, seed, aim=lazy)
    Mp = pairs(M, q)
    k, P = len(q), size * N
    cinv = [_inv(M[O0][7], p) for p in q]
    value = lambda Z: mix_model(A, Z, (Mp[0][O0:O0 + 1], Mp[1][O0:O0 + 1]))[1]["canon_in"][0]

    def solved(residue, top16=False):
        def draw(n):
            Z = _top16(rng, A, (8, k, n)) if top16 else _uniform(rng, A, (8, k, n))
            have = A.canon(value(Z))
            want = np.broadcast_to(np.array([p - 1 if residue else 0 for p in A.q], dtype=U)[:, None], have.shape)
            Z[7] = (Z[7] + _mulmod_rows((want + (A.qa - have)) % A.qa, cinv, A.q)) % A.qa
            return Z
        return draw
    with np.errstate(over="ignore"):
        if lazy:
            lvs, top = _levels(emax["row"]), np.array(emax["one_mix"], dtype=U)[:, None]
            names = ["S_" + n for n in lvs] + ["X_%d" % j for j in range(int(top.max()) + 1)] + ["X_hi_0", "X_hi_qm1", "random"]
            tgt = _rotation(P, names, {0: "X_hi_qm1"})
            X = _uniform(rng, A, (8, k, P))
            for n, lv in lvs.items():
                sel = tgt == names.index("S_" + n)
                for j in range(8):
                    c = _top16(rng, A, (CANDIDATES, k, int(sel.sum())))
                    X[j][:, sel] = _pick(c, A.e(A.mul(c, (Mp[0][O0, j], Mp[1][O0, j]))), lv)
            for j in range(int(top.max()) + 1):
                sel = tgt == names.index("X_%d" % j)
                X[:, :, sel] = _redraw(A, int(sel.sum()), lambda n: _top16(rng, A, (8, k, n)), value, np.minimum(top, U(j)))
            for name, residue in (("X_hi_0", 0), ("X_hi_qm1", 1)):
                sel = tgt == names.index(name)
                X[:, :, sel] = _redraw_max(A, int(sel.sum()), solved(residue, True), value, 8)
        else:
            names = ["C_sum", "C_0", "C_qm1", "random"]
            tgt = _rotation(P, names, {0: "C_qm1"})
            X = _uniform(rng, A, (8, k, P))
            for i, p in enumerate(A.q):
                X[:, i, tgt == 0] = np.array([(p - 1) * _inv(M[O0][j], p) % p for j in range(8)], dtype=U)[:, None]
            for name, residue in (("C_0", 0), ("C_qm1", 1)):
                sel = tgt == names.index(name)
                X[:, :, sel] = solved(residue)(int(sel.sum()))
    _cases[key] = Case(X=X, tgt=tgt, names=names, plan=M, tab=Mp, A=A, size=size, emax=emax)
    return _cases[key]


def count_mix(case, tr, out):
    A, X = case.A, case.X
    res = {}
    if A.lazy:
        hi = (X >= A.qa - A.qa // U(16)).all(axis=0)
        for n, lv in _levels(case.emax["row"]).items():
            res["S_" + n] = ((tr["term_e"][O0] == lv[None]).all(axis=0) & hi).sum(axis=1)
        iv, top = A.units(tr["canon_in"][O0]), np.array(case.emax["one_mix"], dtype=U)[:, None]
        for j in range(int(top.max()) + 1):
            res["X_%d" % j] = np.where(top[:, 0] >= j, (iv == U(j)).sum(axis=1), -1)
        res["X_hi_0"] = ((iv == exit_hi(A, A.one, 0)) & (out[O0] == 0)).sum(axis=1)
        res["X_hi_qm1"] = ((iv == exit_hi(A, A.one, 1)) & (out[O0] == A.qa - U(1))).sum(axis=1)
    else:
        qm1 = A.qa - U(1)
        res["C_sum"] = (tr["acc"][O0] == U(8) * qm1).sum(axis=1)
        res["C_0"], res["C_qm1"] = (out[O0] == 0).sum(axis=1), (out[O0] == qm1).sum(axis=1)
    return {n: [int(v) for v in c] for n, c in res.items()}


# ---- fhe_plane_map -------------------------------------------------------------------------------------------------------------------
PM_IN, PM_T = 70, 64
PM_WIDE, PM_ONLY, PM_SAME = 0, 1, 2       # outputs: 64 distinct sources; the only chunk of 8 terms; eight terms from ONE source (plane 64)
PM_CHUNKS = (0, 3, 7)                     # the first, a middle and the last chunk of the 64-term output


def pm_plan(A, t, emax, seed=SEED, aim=True):
    """taps, weights [9][64], order.  Output 0: planes 0 .. 63, negative weights.  1: planes 0 .. 7 (one chunk), negative.  2: plane 64
    eight times (one LDS row read eight times in a windowed group).  3 .. 6: 1, 9, 16 and 17 live terms on the planes the targets put
    at the bound, so that the (0, 0) padding terms sit beside them.  7, 8: 64 and 23 random terms.  A dead slot's tap points past n_in."""
    rng = np.random.default_rng(seed + 3)
    lim = po.scalar_limit(t)
    n_out = 9
    taps = np.full((n_out, PM_T), PM_IN + 7, dtype=np.uint32)
    w = np.zeros((n_out, PM_T), dtype=np.int64)
    lv = np.minimum(np.array(emax["row"], dtype=np.uint8)[:, None], 2)
    taps[0], w[0] = np.arange(64), _weights(rng, lim, 64, True)
    good = _aimed(rng, A, lim, 32, 15 / 16, 1, lv) if aim else _weights(rng, lim, 32, True)
    for j, c in enumerate(PM_CHUNKS):                                 # the aimed chunks; both ends of the range sit in chunk 1
        w[0, 8 * c:8 * c + 8] = good[8 * j:8 * j + 8]
    w[0, 8], w[0, 9] = -lim, lim
    slots = np.arange(8) * 7 + 2                                      # live slots among dead ones
    taps[1, slots], w[1, slots] = np.arange(8), good[24:]
    taps[2, slots + 1], w[2, slots + 1] = 64, _weights(rng, lim, 8)
    w[2, slots[0] + 1], w[2, slots[1] + 1] = lim, -lim
    taps[3, 40], w[3, 40] = 5, lim
    for o, cnt in ((4, 9), (5, 16), (6, 17)):
        s = np.sort(rng.permutation(PM_T)[:cnt])
        taps[o, s], w[o, s] = np.arange(cnt), _weights(rng, lim, cnt)
    taps[7], w[7] = rng.integers(0, PM_IN, size=64), _weights(rng, lim, 64)
    s = np.sort(rng.permutation(PM_T)[:23])
    taps[8, s], w[8, s] = rng.integers(0, PM_IN, size=23), _weights(rng, lim, 23)
    assert sorted(set((w != 0).sum(axis=1))) == [1, 8, 9, 16, 17, 23, 64]
    return taps, w, rng.permutation(n_out).astype(np.uint32)


def craft_pm(q, lazy, size=2, t=po.T33, seed=SEED, emax=None):
    """one frame of 70 planes: Case(X [70, k, P], ...)"""
    key = ("pm", tuple(q), lazy, size, t, seed, _frozen(emax))
    if key in _cases:
        return _cases[key]
    A = Arith(q, lazy)
    rng = np.random.default_rng(seed + 7 + size)
    emax = emax or (reach_excess(q, t) if lazy else {s_: [2] * len(q) for s_ in SITES})
    taps, w, order = pm_plan(Arith(q, True), t, emax, seed, aim=lazy)
    tab = pm_tab(q, taps, w)
    k, P = len(q), size * N
    wide, only, same = tab[PM_WIDE], tab[PM_ONLY], tab[PM_SAME]
    pr = lambda T, j: (T[1][0][j], T[1][1][j])
    wsum = [sum(int(v) for v in w[PM_SAME]) % p for p in q]
    assert all(wsum), "the eight weights of the one-source output sum to 0 modulo a prime: another seed"

    def out_of(o, Z):
        """(the word entering canon, the trace) of output o alone"""
        _, trs = pm_model(A, Z, [tab[o]])
        return trs[0]["canon_in"], trs[0]

    def set_residue(Z, o, plane, weight, residue):
        """plane `plane` of Z, a term of output o with `weight`, moved so that the output is 0 or q - 1"""
        have = A.canon(out_of(o, Z)[0])
        want = np.broadcast_to(np.array([p - 1 if residue else 0 for p in A.q], dtype=U)[:, None], have.shape)
        Z[plane] = (Z[plane] + _mulmod_rows((want + (A.qa - have)) % A.qa, [_inv(weight, p) for p in q], A.q)) % A.qa
        return Z

    def chunk_values(n, residue=1):
        """the 64-term output with every reduced chunk q - 1 (residue = 1) or 0 (residue = 0: every chunk sum a multiple of q, which the
        lazy product by 1 returns as exactly q): the first source of each chunk is solved"""
        Z = _top16(rng, A, (PM_IN, k, n))
        for c in range(8):
            acc = A.mul(Z[8 * c:8 * c + 8], (wide[1][0][8 * c:8 * c + 8], wide[1][1][8 * c:8 * c + 8])).sum(axis=0, dtype=U)
            have = A.canon(A.mul(acc, A.one)) if A.lazy else A.mul(acc, A.one)
            d = _mulmod_rows(((A.qa - U(1) if residue else U(0) * A.qa) + (A.qa - have)) % A.qa, [_inv(w[0, 8 * c], p) for p in q], A.q)
            Z[8 * c] = (Z[8 * c] + d) % A.qa
        return Z
    with np.errstate(over="ignore"):
        X = _uniform(rng, A, (PM_IN, k, P))
        if lazy:
            lvs, top = _levels(emax["row"]), np.array(emax["one_total"], dtype=U)[:, None]
            names = (["S_chunk%d_%s" % (c, n) for c in PM_CHUNKS for n in lvs] + ["S_only_" + n for n in lvs] + ["S_values", "S_values_q"] + ["X_%d" % j for j in range(int(top.max()) + 1)]
                     + ["X_hi_0", "X_hi_qm1", "X_same_0", "X_same_qm1", "random"])
            tgt = _rotation(P, names)
            for n, lv in lvs.items():
                for c, T, base, name in [(c, wide, 8 * c, "S_chunk%d_%s" % (c, n)) for c in PM_CHUNKS] + [(0, only, 0, "S_only_" + n)]:
                    sel = tgt == names.index(name)
                    for j in range(base, base + 8):
                        cand = _top16(rng, A, (CANDIDATES, k, int(sel.sum())))
                        X[int(T[0][j])][:, sel] = _pick(cand, A.e(A.mul(cand, pr(T, j))), lv)
            sel = tgt == names.index("S_values")
            X[:, :, sel] = chunk_values(int(sel.sum()))
            sel = tgt == names.index("S_values_q")
            X[:, :, sel] = chunk_values(int(sel.sum()), 0)
            value = lambda Z: out_of(PM_WIDE, Z)[0]
            for j in range(int(top.max()) + 1):
                sel = tgt == names.index("X_%d" % j)
                X[:, :, sel] = _redraw(A, int(sel.sum()), lambda n: _top16(rng, A, (PM_IN, k, n)), value, np.minimum(top, U(j)))
            for name, residue in (("X_hi_0", 0), ("X_hi_qm1", 1)):
                sel = tgt == names.index(name)
                X[:, :, sel] = _redraw_max(A, int(sel.sum()), lambda n: set_residue(_top16(rng, A, (PM_IN, k, n)), PM_WIDE, 63, w[0, 63], residue), value, 4)
        else:
            names = ["C_chunk%d" % c for c in PM_CHUNKS] + ["C_only", "C_values", "C_0", "C_qm1", "X_same_0", "X_same_qm1", "random"]
            tgt = _rotation(P, names)
            for i, p in enumerate(A.q):
                for c, T, base, name in [(c, wide, 8 * c, "C_chunk%d" % c) for c in PM_CHUNKS] + [(0, only, 0, "C_only")]:
                    wrow = w[PM_WIDE] if T is wide else w[PM_ONLY][w[PM_ONLY] != 0]
                    for j in range(base, base + 8):
                        X[int(T[0][j]), i, tgt == names.index(name)] = U((p - 1) * _inv(wrow[j], p) % p)
            sel = tgt == names.index("C_values")
            X[:, :, sel] = chunk_values(int(sel.sum()))
            for name, residue in (("C_0", 0), ("C_qm1", 1)):
                sel = tgt == names.index(name)
                X[:, :, sel] = set_residue(X[:, :, sel], PM_WIDE, 63, w[0, 63], residue)
        for name, residue in (("X_same_0", 0), ("X_same_qm1", 1)):     # eight terms from plane 64: x = target / sum of the weights
            sel = tgt == names.index(name)
            for i, p in enumerate(A.q):
                X[64, i, sel] = U((p - 1 if residue else 0) * _inv(wsum[i], p) % p)
    _cases[key] = Case(X=X, tgt=tgt, names=names, plan=(taps, w, order), tab=tab, A=A, size=size, emax=emax)
    return _cases[key]


def count_pm(case, trs, out):
    A, X = case.A, case.X
    hi = X >= A.qa - A.qa // U(16)
    qm1 = A.qa - U(1)
    wide, only = trs[PM_WIDE], trs[PM_ONLY]
    res = {}
    if A.lazy:
        for n, lv in _levels(case.emax["row"]).items():
            for c in PM_CHUNKS:
                res["S_chunk%d_%s" % (c, n)] = ((wide["term_e"][8 * c:8 * c + 8] == lv[None]).all(axis=0) & hi[8 * c:8 * c + 8].all(axis=0)).sum(axis=1)
            res["S_only_" + n] = ((only["term_e"][:8] == lv[None]).all(axis=0) & hi[:8].all(axis=0)).sum(axis=1)
        res["S_values"] = (A.canon(wide["cv"]) == qm1[None]).all(axis=0).sum(axis=1)
        # all eight chunk values at the largest excess of the per-chunk product by 1: exactly q each, the total 8 q, the output 0
        res["S_values_q"] = ((wide["chunk_e"] == 1).all(axis=0) & (wide["cv"] == A.qa[None]).all(axis=0) & (wide["total"] == U(8) * A.qa) & (out[PM_WIDE] == 0)).sum(axis=1)
        iv, top = A.units(wide["canon_in"]), np.array(case.emax["one_total"], dtype=U)[:, None]
        for j in range(int(top.max()) + 1):
            res["X_%d" % j] = np.where(top[:, 0] >= j, (iv == U(j)).sum(axis=1), -1)
        res["X_hi_0"] = ((iv == exit_hi(A, A.one, 0, 9)) & (out[PM_WIDE] == 0)).sum(axis=1)
        res["X_hi_qm1"] = ((iv == exit_hi(A, A.one, 1, 9)) & (out[PM_WIDE] == qm1)).sum(axis=1)
    else:
        for c in PM_CHUNKS:
            res["C_chunk%d" % c] = (wide["acc"][c] == U(8) * qm1).sum(axis=1)
        res["C_only"] = (only["acc"][0] == U(8) * qm1).sum(axis=1)
        res["C_values"] = (wide["cv"] == qm1[None]).all(axis=0).sum(axis=1)
        res["C_0"], res["C_qm1"] = (out[PM_WIDE] == 0).sum(axis=1), (out[PM_WIDE] == qm1).sum(axis=1)
    res["X_same_0"], res["X_same_qm1"] = (out[PM_SAME] == 0).sum(axis=1), (out[PM_SAME] == qm1).sum(axis=1)
    return {n: [int(v) for v in c] for n, c in res.items()}


# ---- the specification on a crafted case (the GPU tests compare with these, never with the model) --------------------------------------
def spec_block(case):
    return po.block8x8_direct(case.A.q, to_ct(case.X, case.size), *case.plan)


def spec_mix(case, bias=None, t=po.T33):
    return po.channel_mix_direct(case.A.q, t, case.plan, to_ct(case.X, case.size), bias)


def spec_pm(case):
    import planemap_oracle as pmo
    return pmo.plane_map_direct(case.A.q, to_ct(case.X, case.size), case.plan[0], case.plan[1])


# ---- one call for the tests: craft, run the model, count -------------------------------------------------------------------------------
def instances():
    """(kind, arguments) of every crafted call of a base: the four block8x8 plans, channel_mix with m = 8 and 3, plane_map"""
    return [("block", (pre, post)) for pre in (True, False) for post in (True, False)] + [("mix", (8,)), ("mix", (3,)), ("pm", ())]


def craft(kind, q, lazy, args, **kw):
    return {"block": craft_block, "mix": craft_mix, "pm": craft_pm}[kind](q, lazy, *args, **kw)


def run_model(kind, case, A=None, **variant):
    """(out [planes, k, P], trace, the sums of the trace as {site: array in the layout [..., k, P]}) in the arithmetic A (the case's own by default)"""
    A = A or case.A
    with np.errstate(over="ignore"):
        if kind == "block":
            out, tr = block_model(A, case.X, case.tab)
            sums = {"col": tr["mid"], "post" if case.plan[3] is not None else "one_block": tr["o"]}
            return out, tr, sums, tr["canon_in"]
        if kind == "mix":
            out, tr = mix_model(A, case.X, case.tab, **variant)
            return out, tr, {"one_mix": tr["acc"]}, tr["canon_in"]
        out, trs = pm_model(A, case.X, case.tab, **variant)
        multi = [t for t in trs if t["multi"]]
        sums = {"one_chunk": np.concatenate([t["acc"] for t in multi]), "one_total": np.stack([t["total"] for t in trs])}
        return out, trs, sums, np.stack([t["canon_in"] for t in trs])


def count(kind, case, tr, out):
    return {"block": count_block, "mix": count_mix, "pm": count_pm}[kind](case, tr, out)


def spec(kind, case, **kw):
    return {"block": spec_block, "mix": spec_mix, "pm": spec_pm}[kind](case, **kw)


def describe(kind, case):
    """what the extremes tests print: the largest unreduced sum of the model in units of q, and the words per canon() interval"""
    _, _, sums, canon_in = run_model(kind, case)
    A = case.A
    big = max(int(A.units(s).max()) for s in sums.values())
    hist = np.bincount(A.units(canon_in).reshape(-1).astype(np.int64), minlength=4) if A.lazy else np.array([canon_in.size])
    return big, [int(v) for v in hist]
