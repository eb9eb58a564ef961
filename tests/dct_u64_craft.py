"""The fused u64 DCT pair (csrc/dct_u64.hip: k_dct_rows_u64, k_dct_cols_u64) restated at the level of VALUES, one work unit at a time (a
work unit = one half-line of one polynomial at one prime), and ciphertext blocks crafted so that the kernels' exits and lazy ranges meet
the values that random data never produces.  No GPU imports, no library.  tests/test_dct_u64_craft_cpu.py proves in this model what the
crafted inputs reach; tests/test_gpu_dct_u64_extremes.py runs the same blocks through the kernels.

What is modelled: the value of every register, restated from the source (not from the kernels' results): fwd_stage / fwd_stage_pm,
line_half<HALF, RED04>, the scale product, inv_stage with inv_bd and the end-of-pass subtractions, inv_bfly_pm with pm3_plan and
inv_exit_pm, the two exits.  Layout is not modelled (which thread and register hold index j changes no value) except the register
index r = (j >> LO) & 7 of a pass, on which the range plans depend.  The transforms run as one butterfly network over the natural index
(ntt_craft.bflies: stage sigma pairs the indices that differ in bit L - 1 - sigma), which is the network the kernels' passes of three
stages evaluate.

Arithmetic.  A work unit is 4 n coefficients through log2 n stages; in scalar Python integers the families below would take hours, so the
model holds its registers in numpy uint64 arrays and CHECKS what u64() checks on a scalar: every sum asserts that it did not wrap, every
X - Y + off that the true value is not negative, every shift that no bit is lost.  The only arithmetic modulo 2^64 is the multiply-add chain
of mul_shoup_lazy4, as in the kernel; its contract (result - acc below 4q) is asserted on every element, and on the elements with the
largest and smallest operand plus a fixed sample of each call the result is compared with ntt_craft.mul_shoup_lazy4 -- Python integers, with
its assertions on the quotient estimate -- and the pseudo-Mersenne product and fold with test_pm_arithmetic_model.mul_pm / fold_pm.
tests/test_dct_u64_craft_cpu.py compares the array primitives with those scalar ones on edge operands and random ones as well.

Every product asserts the operand contract the source states: mul_pm operands at most PmA::LIM / 16 q (and below 2^62), lazy4 results below
4q.  Every site records (static bound, largest operand seen) in sixteenths of q.
"""
import functools

import numpy as np

import ntt_craft as nc
import slot_craft as sc
from test_pm_arithmetic_model import CLASSES, FOLDED, Pm
from test_pm_arithmetic_model import fold_pm as fold_pm_int
from test_pm_arithmetic_model import mul_pm as mul_pm_int

U = np.uint64
M32, S32 = U(0xFFFFFFFF), U(32)
LE, E = 3, 8
PMA = CLASSES["A"]
PM3_E0, PM3_XB = 64, 192
T_PLAIN = 1 << 14
SEED = 20261
SAMPLE = (1, 7, 64, 333)                                    # positions (modulo the size) compared with the scalar models in every call


# ---- checked 64-bit registers ---------------------------------------------------------------------------------------------------------------
def add(a, b):
    c = a + b
    assert not (c < a).any(), "64-bit register overflow"
    return c


def sub_off(X, Y, off):
    """X - Y + off as the kernels write it; the true value must not be negative nor pass 2^64"""
    t = add(X, off)
    assert (t >= Y).all(), "64-bit register underflow"
    return t - Y


def shl1(x):
    assert not (x >> U(63)).any(), "64-bit register overflow"
    return x << U(1)


def csub(x, c, gt=False):
    c = U(c)
    return np.where(x > c if gt else x >= c, x - c, x)


def _spots(x):
    flat = x.reshape(-1)
    return {int(flat.argmax()), int(flat.argmin())} | {s % flat.size for s in SAMPLE}


def lazy4(x, w, wp, q, acc=None):
    """modarith.h mul_shoup_lazy4 / mul_shoup_lazy4_acc on arrays; w, wp broadcast against x"""
    xl, xh, wl, wh, pl, ph = x & M32, x >> S32, w & M32, w >> S32, wp & M32, wp >> S32
    s = ((xh * pl) >> S32) + ((xl * ph) >> S32)             # __builtin_addc of two high words: the carry is bit 32 of s
    A = add(xh * ph, s)
    nq = U((1 << 64) - q)
    al, ah, nl, nh = A & M32, A >> S32, nq & M32, nq >> S32
    P = al * nl + xl * wl                                   # two wrapping v_mad_u64_u32
    if acc is not None:
        P = P + acc
    C = ah * nl + (al * nh + (xh * wl + xl * wh))
    hi = ((P >> S32) + (C & M32)) & M32
    r = (hi << S32) | (P & M32)
    if acc is None:
        assert (r < U(4 * q)).all(), "lazy4 product outside [0, 4q)"
    else:
        assert (r >= acc).all() and (r - acc < U(4 * q)).all(), "lazy4 product outside [0, 4q) or wrapped"
    xb, wb, pb, rb = np.broadcast_arrays(x, w, wp, r)
    ab = None if acc is None else np.broadcast_to(acc, r.shape).reshape(-1)
    xb, wb, pb, rb = xb.reshape(-1), wb.reshape(-1), pb.reshape(-1), rb.reshape(-1)
    for i in _spots(xb):
        assert int(rb[i]) == nc.mul_shoup_lazy4(int(xb[i]), int(wb[i]), int(pb[i]), q, 0 if ab is None else int(ab[i]))
    return r


def mul_pm(x, w, w2, m):
    """ntt_core.h mul_pm on arrays: w canonical, w2 = w 2^31 mod q; the caller asserts the class's operand limit"""
    assert (x < U(1 << 62)).all(), "mul_pm operand at or above 2^62"
    xl, xh = x & U(0x7FFFFFFF), x >> U(31)
    wl, wh, vl, vh = w & M32, w >> S32, w2 & M32, w2 >> S32
    A = add(xh * vl, xl * wl)
    B = add(xh * vh, add(xl * wh, A >> S32))
    zh = B >> U(m.sh)
    assert (zh <= M32).all(), "32-bit register overflow"
    r = add(zh * U(m.delta), ((B & U(m.mb)) << S32) | (A & M32))
    assert 16 * int(r.max()) < PMA["RQ"] * m.q, "mul_pm result at or above RQ"
    xb, wb, rb = (a.reshape(-1) for a in np.broadcast_arrays(x, w, r))
    for i in _spots(xb):
        assert int(rb[i]) == mul_pm_int(int(xb[i]), int(wb[i]), m)
    return r


def fold_pm(x, m):
    top = (x >> S32) >> U(m.sh)
    r = add(top * U(m.delta), (((x >> S32) & U(m.mb)) << S32) | (x & M32))
    assert 16 * int(r.max()) < FOLDED * m.q
    xb, rb = x.reshape(-1), r.reshape(-1)
    for i in _spots(xb):
        assert int(rb[i]) == fold_pm_int(int(xb[i]), m)
    return r


# ---- geometry: 8 coefficients per thread, register passes of three stages (Sh, p_lo, p_stages, Tw::rb) -------------------------------------
def n_passes(L):
    return (L + LE - 1) // LE


def p_lo(L, P):
    return max(L - LE * P - LE, 0)


def p_stages(L, P):
    return min(LE, L - LE * P)


def rb_of(L, P, u):
    return (L - 1 - (LE * P + u)) - p_lo(L, P)


def inv_bd(L, P, r, Ustage):
    """bound (units of q) of register r after the stages S-1 .. Ustage of inverse pass P"""
    bd = 4 if P == n_passes(L) - 1 else 8
    for u in range(p_stages(L, P) - 1, Ustage - 1, -1):
        bd = 4 if (r >> rb_of(L, P, u)) & 1 else 2 * bd
    return bd


def pm3_plan(L, P):
    """dct_u64.hip pm3_plan.  Returns per (u, r0): (fold_y, fold_x, shift, bound of D, bound of T), the exit folds, the bounds after the
    pass before the exit folds (sixteenths of q), and how many fold_y / fold_x the plan holds"""
    bd = [PM3_E0 if P == n_passes(L) - 1 else PM3_XB] * E
    pl, folds = {}, 0
    for u in range(p_stages(L, P) - 1, -1, -1):
        sigma, rb = LE * P + u, rb_of(L, P, u)
        for r0 in range(E):
            if r0 & (1 << rb):
                continue
            r1 = r0 | (1 << rb)
            fy = fx = False
            if bd[r0] + (16 << nc.clog(bd[r1])) > PMA["LIM"]:
                fy, bd[r1] = True, FOLDED
            if bd[r0] + (16 << nc.clog(bd[r1])) > PMA["LIM"]:
                fx, bd[r0] = True, FOLDED
            sh = nc.clog(bd[r1])
            dbd, tbd = bd[r0] + (16 << sh), bd[r0] + bd[r1]
            folds += fy + fx
            pl[(u, r0)] = (fy, fx, sh, dbd, tbd)
            bd[r0] = PMA["RQ"] if sigma == 0 else tbd
            bd[r1] = PMA["RQ"]
    return pl, [P > 0 and bd[r] > PM3_XB for r in range(E)], bd, folds


def pm3_exit_fold_needed(L, P, r):
    """Is the inv_exit_pm fold of register r after pass P needed for the ranges?  The plan's decisions (folds, shifts) stay as they are;
    the TRUE bounds are tracked without that fold, the next pass entered with the largest of them in every register (the LDS exchange may
    bring any register of pass P into any register of pass P - 1).  Returns None when every difference still stays non-negative and at
    most LIM and nothing wraps -- the fold is then a pure range reduction that changes no output for any legal input --, else the reason."""
    tb = None
    for Pp in range(n_passes(L) - 1, -1, -1):
        pl, fold_exit, _, _ = pm3_plan(L, Pp)
        tb = [PM3_E0] * E if tb is None else [max(tb)] * E
        for u in range(p_stages(L, Pp) - 1, -1, -1):
            sigma, rb = LE * Pp + u, rb_of(L, Pp, u)
            for r0 in range(E):
                if r0 & (1 << rb):
                    continue
                r1 = r0 | (1 << rb)
                fy, fx, sh, _, _ = pl[(u, r0)]
                ty, tx = FOLDED if fy else tb[r1], FOLDED if fx else tb[r0]
                if ty > (16 << sh):
                    return "pass %d stage %d: X - Y + 2^%d q can be negative" % (Pp, u, sh)
                if tx + (16 << sh) > PMA["LIM"] or (sigma == 0 and tx + ty > PMA["LIM"]):
                    return "pass %d stage %d: a product operand can pass LIM" % (Pp, u)
                tb[r0], tb[r1] = PMA["RQ"] if sigma == 0 else tx + ty, PMA["RQ"]
        for k in range(E):
            if fold_exit[k] and not (Pp == P and k == r):
                tb[k] = FOLDED
    return None


def bn(L, body):
    """Bn<L, LAZY, PM>::V: bound (units of q) of the forward transform's outputs"""
    return 2 + (L << PMA["CS"]) if body == "pm" else 2 + 4 * L if body == "lazy" else 8


@functools.lru_cache(maxsize=None)
def stage(L, sigma):
    b = L - 1 - sigma
    j = np.arange(1 << L)
    j0 = j[((j >> b) & 1) == 0]
    return j0, j0 | (1 << b), (1 << sigma) + (j0 >> (b + 1))


class Tab:
    """twiddles of one prime as arrays: (w, Shoup companion, w 2^31 mod q) for both directions"""

    def __init__(self, q, n):
        T = nc.tables(q, n)
        self.q, self.n, self.L, self.pm = q, n, T.L, Pm(q) if 33 <= q.bit_length() <= 63 and ((1 << q.bit_length()) - q) < (1 << 31) else None
        arr = lambda v: np.array(v, dtype=U)
        self.tw, self.twp, self.itw, self.itwp = arr(T.tw), arr(T.twp), arr(T.itw), arr(T.itwp)
        self.tw2, self.itw2 = arr([(w << 31) % q for w in T.tw]), arr([(w << 31) % q for w in T.itw])
        self.one_p = U((1 << 64) // q)


@functools.lru_cache(maxsize=None)
def tab(q, n):
    return Tab(q, n)


class Reach(dict):
    """site -> [static bound, largest operand seen], sixteenths of q"""

    def note(self, site, bound16, v, q, strict=True):
        top = int(v.max())
        assert (16 * top < bound16 * q) if strict else (16 * top <= bound16 * q), "%s: operand above its static bound" % site
        cell = self.setdefault(site, [bound16, 0])
        assert cell[0] == bound16
        cell[1] = max(cell[1], nc.sixteenths(top, q))

    def merge(self, other):
        for k, (b, t) in other.items():
            cell = self.setdefault(k, [b, 0])
            assert cell[0] == b
            cell[1] = max(cell[1], t)


# ---- the kernels' pieces -----------------------------------------------------------------------------------------------------------------------
def fwd_transform(x, T, body, reach):
    """fwd_stage<L, P, U, LAZY> / fwd_stage_pm on x [4, n] (below 2q): the four polynomials of a unit share every twiddle"""
    q, L = T.q, T.L
    q4 = U(4 * q)
    for sigma in range(L):
        j0, j1, ti = stage(L, sigma)
        X, Y = x[:, j0], x[:, j1]
        if body == "pm":
            bd = 32 + (sigma << (4 + PMA["CS"]))
            assert bd <= PMA["LIM"]
            reach.note("rows fwd", PMA["LIM"], Y, q, strict=False)
            reach.note("rows fwd stage %d" % sigma, bd, np.maximum(X, Y), q, strict=False)
            t = mul_pm(Y, T.tw[ti], T.tw2[ti], T.pm)
            x[:, j0], x[:, j1] = add(X, t), sub_off(X, t, U(q << PMA["CS"]))
        else:
            if body == "lazy":
                reach.note("rows fwd stage %d" % sigma, 16 * (2 + 4 * sigma), np.maximum(X, Y), q)
            else:
                reach.note("rows fwd stage %d" % sigma, 128, np.maximum(X, Y), q)
                X = csub(X, 4 * q)
            S = lazy4(Y, T.tw[ti], T.twp[ti], q, acc=X)
            x[:, j0], x[:, j1] = S, sub_off(shl1(X), S, q4)
    reach.note("rows fwd out", 16 * bn(L, body), x, q, strict=body != "pm")
    return x


def line_half(x, half, red04, B, T, C, reach, tag, skip_static=False):
    """line_half<HALF, RED04>: x [4, n] below B q -> the four outputs 2m + HALF.  C[cid] = (w, companion) arrays over the slots"""
    q = T.q
    assert skip_static or 4 * B * q < 1 << 64, "the caller's condition 4 B q < 2^64"
    sub = U(B * q)
    MUL = lambda v, cid: lazy4(v, C[cid][0], C[cid][1], q)
    x0, x1, x2, x3 = x
    assert (x < U(B * q)).all(), "%s: line input at or above B q" % tag
    if half == 0:
        tmp10, tmp13, tmp11, tmp12 = add(x0, x3), sub_off(x0, x3, sub), add(x1, x2), sub_off(x1, x2, sub)
        s = add(tmp12, tmp13)
        reach.note(tag + " tmp12+tmp13", 64 * B, s, q)
        z1 = MUL(s, 0)
        o0, o4 = add(tmp10, tmp11), sub_off(tmp10, tmp11, U(2 * B * q))
        reach.note(tag + " out 0", 64 * B, o0, q)
        reach.note(tag + " out 4", 64 * B, o4, q)
        if red04:
            one = U(1)
            o0, o4 = lazy4(o0, one, T.one_p, q), lazy4(o4, one, T.one_p, q)
        o2, o6 = add(z1, MUL(tmp13, 1)), add(z1, MUL(tmp12, 2))
        assert (o2 < U(8 * q)).all() and (o6 < U(8 * q)).all()
        return [o0, o2, o4, o6]
    tmp7, tmp6, tmp5, tmp4 = x0, x1, x2, x3
    z1, z2, z3, z4 = add(tmp4, tmp7), add(tmp5, tmp6), add(tmp4, tmp6), add(tmp5, tmp7)
    s = add(z3, z4)
    reach.note(tag + " z3+z4", 64 * B, s, q)
    z5 = MUL(s, 3)
    t4, t5, t6, t7 = MUL(tmp4, 4), MUL(tmp5, 5), MUL(tmp6, 6), MUL(tmp7, 7)
    m1, m2, m3, m4 = MUL(z1, 8), MUL(z2, 9), add(MUL(z3, 10), z5), add(MUL(z4, 11), z5)
    outs = [add(add(t7, m1), m4), add(add(t6, m2), m3), add(add(t5, m2), m4), add(add(t4, m1), m3)]
    assert all((o < U(16 * q)).all() for o in outs)
    return outs


def rows_unit(A, Bq, half, T, body, C, reach, var=None):
    """rows_body<L, HALF, LAZY, PM>: A[m], Bq[m] = the canonical coefficients of ciphertexts m and 7 - m of the line ([4, n]);
    returns the row outputs 2m + HALF as the kernel stores them (below 16 q)"""
    var = var or {}
    assert (A < U(T.q)).all() and (Bq < U(T.q)).all()
    x = sub_off(A, Bq, U(T.q)) if half else add(A, Bq)
    x = fwd_transform(x.copy(), T, body, reach)
    outs = np.stack(line_half(x, half, not var.get("no_red04"), bn(T.L, body), T, C, reach, "rows", bool(var.get("skip_static"))))
    return outs


def inv_shoup(x, T, reach, var):
    """inv_stage<L, P, U> over all passes: x [4, n] below 4q -> below 4q"""
    q, L = T.q, T.L
    NP = n_passes(L)
    assert 128 * q < 1 << 64 and (x < U(4 * q)).all()
    for P in range(NP - 1, -1, -1):
        LO = p_lo(L, P)
        for u in range(p_stages(L, P) - 1, -1, -1):
            sigma = LE * P + u
            j0, j1, ti = stage(L, sigma)
            bds = np.array([inv_bd(L, P, r, u + 1) for r in range(E)], dtype=np.int64)
            bd = bds[(j1 >> LO) & 7]
            assert (bd == bds[(j0 >> LO) & 7]).all() and set(bds.tolist()) <= {4, 8, 16, 32}
            shift = np.where(bd == 4, 0, np.where(bd == 8, 1, np.where(bd == 16, 2, 3)))
            if var.get("off_small") is not None:             # the offset of one class taken one class too small
                shift = np.where(bd == var["off_small"], shift - 1, shift)
                assert (shift >= 0).all()
            off = U(4 * q) << shift.astype(U)
            X, Y = x[:, j0], x[:, j1]
            lim = bd.astype(U) * U(q)
            assert (X < lim).all() and (Y < lim).all(), "inverse stage %d: register above its tracked bound" % sigma
            Tm, D = add(X, Y), sub_off(X, Y, off)
            for c in sorted(set(bd.tolist())):
                sel = bd == c
                reach.note("inv difference, bound %d q" % (2 * c), 32 * c, D[:, sel], q)
                reach.note("inv sum, bound %d q" % (2 * c), 32 * c, Tm[:, sel], q)
            x[:, j0] = lazy4(Tm, T.itw[0], T.itwp[0], q) if sigma == 0 else Tm
            x[:, j1] = lazy4(D, T.itw[ti], T.itwp[ti], q)
        if P > 0:
            r = (np.arange(1 << L) >> LO) & 7
            bd0 = np.array([inv_bd(L, P, k, 0) for k in range(E)], dtype=np.int64)[r]
            for ci, (above, c) in enumerate(((32, 32), (16, 16), (8, 8))):
                if var.get("drop_csub") == (P, ci):
                    continue
                x = np.where((bd0 > above)[None, :], csub(x, c * q), x)
            assert (x < U(8 * q)).all(), "register at or above 8q after the end-of-pass subtractions"
    assert (x < U(4 * q)).all()
    return x


def inv_pm(x, T, reach, var):
    """inv_bfly_pm / inv_exit_pm over all passes: x [4, n] below 4q -> mul_pm results (below RQ / 16 q)"""
    q, L, m = T.q, T.L, T.pm
    NP = n_passes(L)
    assert 16 * int(x.max()) <= PM3_E0 * q
    dropped = var.get("drop_fold") is not None               # the wrong variant keeps the hard contracts only: no wrap, product operands within LIM
    for P in range(NP - 1, -1, -1):
        LO = p_lo(L, P)
        pl, fold_exit, bd_out, _ = pm3_plan(L, P)
        if var.get("drop_fold") is not None and var["drop_fold"][0] == P:      # one inv_exit_pm fold left out; the next pass goes on as planned
            fold_exit = [f and r != var["drop_fold"][1] for r, f in enumerate(fold_exit)]
        for u in range(p_stages(L, P) - 1, -1, -1):
            sigma = LE * P + u
            j0, j1, ti = stage(L, sigma)
            r0 = (j0 >> LO) & 7
            X, Y = x[:, j0].copy(), x[:, j1].copy()
            D, Tm = np.empty_like(X), np.empty_like(X)
            for r in sorted(set(r0.tolist())):
                fy, fx, sh, dbd, tbd = pl[(u, r)]
                sel = r0 == r
                Xs, Ys = X[:, sel], Y[:, sel]
                if fy:
                    Ys = fold_pm(Ys, m)
                if fx:
                    Xs = fold_pm(Xs, m)
                t, d = add(Xs, Ys), sub_off(Xs, Ys, U(q << sh))
                assert dbd <= PMA["LIM"]
                reach.note("inv difference (pm)", PMA["LIM"], d, q, strict=False)
                assert dropped or (16 * int(d.max()) <= dbd * q and 16 * int(t.max()) <= tbd * q), "inverse stage %d: operand above its planned bound" % sigma
                if sigma == 0:
                    assert tbd <= PMA["LIM"]
                D[:, sel], Tm[:, sel] = d, t
            x[:, j0] = mul_pm(Tm, T.itw[0], T.itw2[0], m) if sigma == 0 else Tm
            x[:, j1] = mul_pm(D, T.itw[ti], T.itw2[ti], m)
        if P > 0:
            r = (np.arange(1 << L) >> LO) & 7
            fe = np.array(fold_exit)[r]
            if fe.any():
                x[:, fe] = fold_pm(x[:, fe], m)
            assert dropped or 16 * int(x.max()) <= PM3_XB * q, "register above XB after the exit folds"
    return x


def cols_unit(A, Bq, half, col, T, pm, C, S, reach, var=None):
    """cols_body<L, HALF, PM>: A[m], Bq[m] = the intermediates of rows m and 7 - m at this column ([4, n], below 16 q); S[row] = (scale,
    companion) of output (row, col).  Returns (canonical outputs 2m + HALF [4, n], the lazy values in front of the exit: in front of
    csub(csub(., 2q), q), or fold_pm's result in front of csub(., q))"""
    var = var or {}
    q = T.q
    assert (A < U(16 * q)).all() and (Bq < U(16 * q)).all(), "intermediate at or above 16 q"
    x = sub_off(A, Bq, U(16 * q)) if half else add(A, Bq)
    outs = line_half(x, half, False, 32, T, C, reach, "cols")
    y = []
    for mi, o in enumerate(outs):
        reach.note("cols scale operand", 2048, o, q)
        y.append(lazy4(o, S[2 * mi + half][0], S[2 * mi + half][1], q))
    y = np.stack(y)
    gt = var.get("exit_gt", -1)
    if pm:
        v = fold_pm(inv_pm(y, T, reach, var), T.pm)
        return csub(v, q, gt == 0), v
    v = inv_shoup(y, T, reach, var)
    return csub(csub(v, 2 * q, gt == 0), q, gt == 1), v


# ---- the class rule of fhe_build_base / fhe_dct_u64_supported / fhe_dct_u64_launch ---------------------------------------------------------------
def pm_class(primes):
    """csrc/fhe_hip.hip fhe_build_base: 1 = class A (every prime 52..55 bits), 2 = class B, 0 = neither"""
    a_all = b_all = True
    for q in primes:
        b = q.bit_length()
        if b < 34 or b > 58:
            return 0
        delta = (1 << b) - q
        prod, folded, vv = (1 << b) + (delta << 32), (1 << b) + (delta << (64 - b)), (1 << b) + (delta << (85 - b))
        if delta >> 31 or folded * 16 > q * FOLDED:
            return 0
        a_all = a_all and 52 <= b <= 55 and prod * 16 <= q * PMA["RQ"] and vv * 16 <= q * PMA["RQ"]
        b_all = b_all and b >= 52 and prod * 16 <= q * CLASSES["B"]["RQ"] and vv * 16 <= q * CLASSES["B"]["RQ"]
    return 1 if a_all else 2 if b_all else 0


def classify(n, primes, switches=None, lazy_limit=56):
    """-> (path of fhe_dct_path, body of the rows, PM columns, fhe_arith_path & 3).  path 2 = the fused u64 pair: no prime size the
    exact-FP64 pair takes (below 2^47), at most 57 bits, n in {2048, 4096, 8192}.  LAZY up to 56 bits, PM for class A without
    FHE_NTT_NOPM.  lazy_limit = 57: the deliberately wrong rule."""
    switches = switches or {}
    bits, L = max(p.bit_length() for p in primes), n.bit_length() - 1
    cls, nopm = pm_class(primes), bool(switches.get("FHE_NTT_NOPM"))
    arith = 0 if nopm else cls
    if switches.get("FHE_DCT_FORCE_U64") or bits > 57 or L not in (11, 12, 13):
        return 0, None, None, arith
    if bits <= 47:
        return 1, None, None, arith
    pm = cls == 1 and not nopm
    return 2, "pm" if pm else "lazy" if bits <= lazy_limit else "nolazy", pm, arith


def static_bounds_hold(L, body, q):
    """the two conditions of the file's header: 4 Bn q < 2^64 (row line_half) and 128 q < 2^64 (column line_half, inv_stage)"""
    return 4 * bn(L, body) * q < 1 << 64 and 128 * q < 1 << 64


# ---- contexts of tests/test_gpu_dct_u64_extremes.py ----------------------------------------------------------------------------------------------
PRESET = [0x7FFFFFFF380001, 0x3FFFFFFF000001]               # SEAL 2.3 coeff_modulus_128 as SEAL23_2048 / SEAL23_4096 / P8192 use it
PRESET3 = [0x7FFFFFFF380001, 0x7FFFFFFEF00001, 0x3FFFFFFF000001]
NOPM = {"FHE_NTT_NOPM": 1}


def next_prime_above(p, step=1 << 14):
    p += step
    while not sc.is_prime(p):
        p += step
    return p


def top_primes(bits):
    """the largest prime of `bits` bits that is 1 (mod 2^14), an NTT prime up to n = 8192"""
    return nc.largest_primes(bits, 8192, 1)[0]


LAZY56 = [top_primes(56), top_primes(55)]
NOLAZY57 = [top_primes(57), top_primes(56)]
LOW48 = [sc.P_ABOVE_47, next_prime_above(sc.P_ABOVE_47)]


def _contexts():
    out = {}
    for n in (2048, 4096, 8192):
        for name, q, sw in (("pmA", PRESET, {}), ("shoup55", PRESET, NOPM), ("lazy56", LAZY56, {}), ("nolazy57", NOLAZY57, {})):
            out["%s-n%d" % (name, n)] = (n, q, T_PLAIN, dict(sw))
    out["low48-n4096"] = (4096, LOW48, T_PLAIN, {})
    out["pmA-k3-n2048"] = (2048, PRESET3, T_PLAIN, {})        # base sizes 3 and 1: decode() divides the grid by k
    out["nolazy57-k1-n2048"] = (2048, NOLAZY57[:1], T_PLAIN, {})
    return {k: v + (classify(v[0], v[1], v[3])[1:3],) for k, v in out.items()}


CONTEXTS = _contexts()                                      # name -> (n, primes, t, switches, expected (rows body, PM columns))


def instantiations(names=None):
    """the (kernel, L, LAZY, PM) instantiations the contexts launch"""
    out = set()
    for name in names or CONTEXTS:
        n, q, _, sw, (body, pm) = CONTEXTS[name]
        L = n.bit_length() - 1
        out.add(("rows", L, body != "nolazy", body == "pm"))
        out.add(("cols", L, pm))
    return out


ALL_INSTANTIATIONS = {("rows", L, lazy, pm) for L in (11, 12, 13) for lazy, pm in ((True, True), (True, False), (False, False))} | \
                     {("cols", L, pm) for L in (11, 12, 13) for pm in (True, False)}


# ---- the unit model bound to one (n, primes): constants in the network's slot order ---------------------------------------------------------------
class Model:
    """sm: slot_craft.SlotModel of the same (n, primes) (the constants' slot values in the oracle's order); the permutation to the
    network's order comes from the transform of the monomial X in both (ntt_craft.slot_permutation)"""

    def __init__(self, sm):
        self.sm, self.n, self.k, self.q = sm, sm.n, sm.k, list(sm.q)
        self.L = self.n.bit_length() - 1
        self.T = [tab(q, self.n) for q in self.q]
        self.C, self.S = [], []
        mono = np.zeros(self.n, dtype=U)
        mono[1] = 1
        for i, q in enumerate(self.q):
            perm = nc.slot_permutation(nc.exact_fwd([0, 1] + [0] * (self.n - 2), nc.tables(q, self.n)), sm.orc.ntt_fwd(mono, i))
            comp = lambda w: np.array([(int(v) << 64) // q for v in w], dtype=U)
            self.C.append([(sm.C[c, i][perm], comp(sm.C[c, i][perm])) for c in range(12)])
            self.S.append([[(sm.fwd_scale[r, c, i][perm], comp(sm.fwd_scale[r, c, i][perm])) for c in range(8)] for r in range(8)])

    def rows(self, block, i, poly, line, half, body, reach, var=None):
        A = np.stack([block[8 * line + m, poly, i] for m in range(4)])
        B = np.stack([block[8 * line + 7 - m, poly, i] for m in range(4)])
        return rows_unit(A, B, half, self.T[i], body, self.C[i], reach, var)

    def run(self, block, body, pm, units=None, var=None):
        """block [64, 2, k, n] canonical coefficients; units: iterable of (prime, poly, column, half), default all.  Returns
        (out {unit: canonical [4, n] = outputs (2m + half, column)}, lazy {unit: [4, n]}, Reach)"""
        reach, mid, out, lazy = Reach(), {}, {}, {}
        units = list(units) if units is not None else [(i, p, c, h) for i in range(self.k) for p in range(2) for c in range(8) for h in range(2)]
        for i, p, c, h in units:
            for line in range(8):                             # column c needs the row outputs of parity c & 1 of every line
                key = (i, p, line, c & 1)
                if key not in mid:
                    mid[key] = self.rows(block, i, p, line, c & 1, body, reach, var)
            row = lambda r: mid[(i, p, r, c & 1)][c >> 1]
            A, B = np.stack([row(m) for m in range(4)]), np.stack([row(7 - m) for m in range(4)])
            out[(i, p, c, h)], lazy[(i, p, c, h)] = cols_unit(A, B, h, c, self.T[i], pm, self.C[i], [self.S[i][r][c] for r in range(8)], reach, var)
        return out, lazy, reach

    @staticmethod
    def expected(want, unit):
        """the rows of an oracle output block [64, 2, k, n] that unit (prime, poly, column, half) computes: [4, n]"""
        i, p, c, h = unit
        return np.stack([want[8 * (2 * m + h) + c, p, i] for m in range(4)])


# ---- the families -------------------------------------------------------------------------------------------------------------------------------
Z_NAMES = ("one", "half-", "half+", "top")


def z_constant(q, name):
    return {"one": 1, "half-": (q - 1) // 2, "half+": (q + 1) // 2, "top": q - 1}[name]


def x_targets(q, n, seed=SEED):
    """[64, k, n]: every coefficient of every output polynomial (polynomial 0) drawn from the targets"""
    out = np.empty((64, len(q), n), dtype=U)
    for i, p in enumerate(q):
        rng = np.random.default_rng([seed, n, i])
        out[:, i] = np.array(nc.targets(p), dtype=U)[rng.integers(0, 7, size=(64, n))]
    return out


def craft_x(sm, seed=SEED):
    """the block whose 64 output polynomials are x_targets (polynomial 1: their negation): forward NTT of the target, the scale undone,
    the 4 x 4 systems of the column and the row halves solved per slot.  Returns (block [64, 2, k, n], targets)"""
    tg = x_targets(sm.q, sm.n, seed)
    G = np.stack([np.stack([sm.orc.ntt_fwd(tg[o, i], i) for i in range(sm.k)]) for o in range(64)]).reshape(8, 8, sm.k, sm.n)
    X, ok = sm.craft_fwd_f4(G)
    assert ok.all(), "%d slots left unsolved: one free slot un-prescribes every coefficient" % int((~ok).sum())
    return sm.block((X, ok), np.random.default_rng(seed)), tg


W_SIGNS = {"same": lambda r, c: 0, "col-alt": lambda r, c: c & 1, "row-alt": lambda r, c: r & 1, "checker": lambda r, c: (r ^ c) & 1,
           "col-half": lambda r, c: c >> 2, "row-half": lambda r, c: r >> 2}
W_POLYS = ("all q-1", "all q/2", "0, q-1 alternating", "(q-1) X^0", "(q-1) X^%d")           # of ntt_craft.structured; %d: n - 1
W_RANDOM = 4


def w_names(n):
    return ["%s / %s" % (p % (n - 1) if "%d" in p else p, s) for p in W_POLYS for s in W_SIGNS] + ["random %d" % r for r in range(W_RANDOM)]


def w_block(sm, name, seed=SEED):
    """one candidate of the W search: every ciphertext holds the same structured polynomial (ntt_craft.structured), negated where the
    block-level sign pattern says so (polynomial 1 is the negation of polynomial 0), or a random block with a fixed seed"""
    n, k, q = sm.n, sm.k, sm.q
    if name.startswith("random "):
        return sm.orc.random_ct(64, seed=seed + 100 + int(name.split()[1]))
    poly, sign = name.split(" / ")
    blk = np.zeros((64, 2, k, n), dtype=U)
    for i, p in enumerate(q):
        v = np.array(dict(nc.structured(p, n))[poly], dtype=U)
        neg = (U(p) - v) % U(p)
        for ct in range(64):
            s = W_SIGNS[sign](ct >> 3, ct & 7)
            blk[ct, 0, i], blk[ct, 1, i] = (neg, v) if s else (v, neg)
    return blk


W_SITES = ("rows tmp12+tmp13", "rows out 0", "rows out 4", "cols tmp12+tmp13", "cols out 0", "cols out 4")


def w_score(reach):
    """the three sites of the search: the row line_half sums, the column line_half sums in front of the scale product, the inv_stage
    differences (Shoup) -- each as the share of its static bound that was reached"""
    share = lambda keys: max([reach[k][1] / reach[k][0] for k in keys if k in reach] or [0.0])
    return (share([s for s in W_SITES if s.startswith("rows")]), share([s for s in W_SITES if s.startswith("cols")]),
            share([s for s in reach if s.startswith("inv difference")]))


W_UNITS = [(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0), (0, 0, 1, 1)]


def search_w(model, body, pm, seed=SEED):
    """bounded search in the model: every candidate through the units (prime 0, polynomial 0, columns 0 and 1, both halves) -- 16 row and 4
    column units.  Returns {name: (share of the row bound, of the column bound, of the inverse difference bound)}"""
    return {nm: w_score(model.run(w_block(model.sm, nm, seed), body, pm, units=W_UNITS)[2]) for nm in w_names(model.n)}


def craft_batch(sm, seed=SEED):
    """the batch of one (n, primes): names, blocks [9, 64, 2, k, n], the X targets [64, k, n].  The W block is the candidate W_CHOICE names
    for the prime set: the winner of search_w at n = 2048, summed over the bodies that run those primes (tests/test_dct_u64_craft_cpu.py
    repeats the search); at n = 4096 and 8192 the same candidate is taken without a search and what it reaches is measured."""
    q, n, k = sm.q, sm.n, sm.k
    top = np.zeros((64, 2, k, n), dtype=U)
    for i, p in enumerate(q):
        top[:, :, i, :] = p - 1
    blocks = [("G-random", sm.orc.random_ct(64, seed=seed)), ("G-top", top), ("G-zero", np.zeros((64, 2, k, n), dtype=U))]
    for nm in Z_NAMES:
        blocks.append(("Z-" + nm, sm.constant_block([[z_constant(p, nm) for p in q]] * 64)))
    xb, tg = craft_x(sm, seed)
    blocks.append(("X", xb))
    blocks.append(("W", w_block(sm, w_choice(q, n), seed)))
    return [a for a, _ in blocks], np.stack([b for _, b in blocks]), tg


W_CHOICE = {55: "random 3", 56: "all q-1 / row-alt", 57: "all q/2 / row-alt", 48: "(q-1) X^0 / row-alt"}   # max bits of the prime set -> candidate


def w_choice(q, n):
    name = W_CHOICE[max(p.bit_length() for p in q)]
    return name % (n - 1) if "%d" in name else name


def z_expected(sm, name, quant):
    """closed form of a constant block: DC output 64 c encode(0.125) encode(1 / Q[0]), the other 63 ciphertexts zero"""
    orc = sm.orc
    dc = np.zeros((2, sm.k, sm.n), dtype=U)
    for i, p in enumerate(sm.q):
        c = z_constant(p, name)
        dc[0, i, 0], dc[1, i, 0] = 64 * c % p, -64 * c % p
    out = np.zeros((64, 2, sm.k, sm.n), dtype=U)
    out[0] = orc.multiply_plain(orc.multiply_plain(dc, orc.encode(0.125)), orc.encode(1 / float(quant[0])))
    return out


def slot_model(oracle_mod, n, q, t=T_PLAIN):
    return sc.SlotModel(oracle_mod.Oracle(n, list(q), t), oracle_mod.YQT)
