"""The integer JPEG kernels restated at the level of VALUES, and ciphertext blocks crafted so that their exits and canonical ties meet the
values random data never produces.  No GPU imports, no library.  tests/test_jpeg_u64_craft_cpu.py proves in these models what the crafted
inputs reach; tests/test_gpu_jpeg_u64_extremes.py runs the same blocks through the kernels.

What is modelled, word for word from the source:
  csrc/idct.hip     idct_line_pm<I> with both k_idct_lines_pm bodies (input-scale product in the rows, canon_pm in the columns);
                    idct_line_u64 / k_idct_slots; the tail of k_ycc2rgb
  csrc/fhe_hip.hip  dct_line_pm<I> with both k_dct_lines_pm bodies (scale product and canon_pm in the columns); dct_line_u64 /
                    k_dct_slots; k_rgb_combine_pm for both classes; the exit of k_rgb_ntt_pm<.., true>; the tail of k_rgb2ycc
Each line is ONE function over an `ops` object, so the same dataflow runs on
  PmOps   lazy 64-bit registers (numpy uint64): every sum asserts that it did not wrap, every X - Y + off that it is not negative, every
          product is mulvv_pm(fold_pm(x), c) on arrays, compared with test_pm_arithmetic_model's Python integers on the largest and the
          smallest operand and a fixed sample of every call; every site records (static bound, largest value seen)
  CanOps  canonical residues (addmod / submod / mul_shoup as residue arithmetic) with selectable wrong comparisons, counting the ties
  IvOps   intervals in units of q: the static bounds of the source's comments, and the same with the product bound that mulvv_pm really
          has (2^b + 2 delta^2, csrc/ntt_core.h) and the structure of the column inputs -- what decides which difference offsets are slack
The transforms around the slot kernels are the oracle's (slot_craft.SlotModel); the models are slotwise, so the slot order does not matter.
The pseudo-Mersenne colour path runs ntt_craft.pm_forward_lazy / pm_inverse_lazy (Python integers, the network's order) around the
combine step; its inverse instantiation ntt_inv_regs_pm<L, 1, rgb_sum_bound(RQ), ..> is the model's e0 = rgb_sum_bound(RQ).

The words a line or slot kernel stores are not what a caller gets: an inverse transform runs on them.  transform_entry_wraps restates the
one place where a stored word that is congruent but not canonical can change a ciphertext (the first butterfly of k_ntt_inv_pm), and
e_targets puts operands there.

Wrong variants (VARIANTS): each is a switch of a model, never of a kernel."""
from collections import Counter

import numpy as np

import dct_u64_craft as dc
import modswitch_oracle as mo
import ntt_craft as nc
import slot_craft as sc
from dct_u64_craft import NOPM, PRESET3, Reach
from test_pm_arithmetic_model import CLASSES, FOLDED, Pm
from test_pm_arithmetic_model import mulvv_pm as mulvv_pm_int

U = np.uint64
M32, S32 = U(0xFFFFFFFF), U(32)
T_PLAIN = 1 << 14
N = 1024
SEED = 20262
FORCE_U64 = {"FHE_DCT_FORCE_U64": 1}
RGB_CONSTS = (0.299, 0.587, 0.114, -0.168736, 0.331264, 0.5, 0.5, 0.418688, 0.081312)
YCC_CONSTS = (1.402, 0.344136, 0.714136, 1.772)
VARIANTS = ("exit_no_csub", "exit_gt", "addmod_gt", "submod_neg0", "offset_on_poly1", "offset_sign", "offset_too_small")


# ---- the class-A base with the widest delta --------------------------------------------------------------------------------------------------
def admits_class_a(q):
    """csrc/fhe_hip.hip fhe_build_base for one prime of class A: delta below 2^31, fold_pm's result below 17/16 q, mul_pm's and
    mulvv_pm's results below RQ = 6 q"""
    b = q.bit_length()
    delta = (1 << b) - q
    folded, prod, vv = (1 << b) + (delta << (64 - b)), (1 << b) + (delta << 32), (1 << b) + (delta << (85 - b))
    return 52 <= b <= 55 and not delta >> 31 and folded * 16 <= q * FOLDED and prod * 16 <= q * CLASSES["A"]["RQ"] and vv * 16 <= q * CLASSES["A"]["RQ"]


def widest_delta_prime(bits, step=1 << 14):
    """the smallest prime of `bits` bits, 1 (mod 2^14), that fhe_build_base admits to class A: the three inequalities only tighten as delta
    grows, so the largest admitted delta is found by bisection and the first admitted prime at or above 2^bits - delta is taken"""
    lo, hi = 1, (1 << (bits - 1)) - 1
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if admits_class_a((1 << bits) - mid) else (lo, mid - 1)
    q = (1 << bits) - lo
    q += -(q - 1) % step
    while not (admits_class_a(q) and sc.is_prime(q)):
        q += step
    return q


WIDE = [0x7FFFFFFD80C001, 0xFFFFFFFD98001]                    # widest_delta_prime(55), widest_delta_prime(52): delta = 41 893 887 and 2 523 135


def bases(n=N):
    """name -> (n, primes, switches of the default context, pseudo-Mersenne class the kernels run on: "A", "B" or None)"""
    if n == N:
        return {"pmA": (n, list(PRESET3), {}, "A"), "nopm": (n, list(PRESET3), dict(NOPM), None), "Q58": (n, mo.bases(n)["Q58"], {}, "B"),
                "Q61": (n, mo.bases(n)["Q61"], {}, None), "wide": (n, list(WIDE), {}, "A")}
    return {"pmA": (n, list(PRESET3), {}, "A"), "nopm": (n, list(PRESET3), dict(NOPM), None), "Q58": (n, mo.primes_below(58, n, 2), {}, "B")}


def expected_paths(n, q, switches):
    """(fhe_dct_path, fhe_arith_path & 3) by the rule restated in dct_u64_craft.classify"""
    path, _, _, arith = dc.classify(n, q, switches)
    return path, arith


def slot_model(oracle_mod, n, q, t=T_PLAIN):
    return sc.SlotModel(oracle_mod.Oracle(n, list(q), t), oracle_mod.YQT)


# ---- checked registers -------------------------------------------------------------------------------------------------------------------------
def pow2_at_least(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def idct_pm_out(I):
    return I + pow2_at_least(I) + 48


def mulvv_pm(a, b, m):
    """ntt_core.h mulvv_pm on arrays: a below 2^(b+1) (a folded value), b canonical.  The result is asserted below 2^b + 2 delta^2, the
    bound the header derives (the class's RQ is checked by the caller's Reach)"""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=U), np.asarray(b, dtype=U))
    assert (a < U(1 << (m.b + 1))).all() and (b < U(m.q)).all(), "mulvv_pm operand out of range"
    al, ah, bl, bh = a & M32, a >> S32, b & M32, b >> S32
    P0 = al * bl
    mid = dc.add(ah * bl, dc.add(al * bh, P0 >> S32))
    top = dc.add(ah * bh, mid >> S32)
    sh, mb, dl = U(m.sh), U(m.mb), U(m.delta)
    zh_lo = ((((top & M32) << S32) | (mid & M32)) >> sh) & M32
    zh_hi = top >> sh
    assert (zh_hi <= M32).all(), "32-bit register overflow"
    zl = (P0 & M32) | (((mid & M32) & mb) << S32)
    F = dc.add(zh_lo * dl, zl)
    G = dc.add(zh_hi * dl, F >> S32)
    zh2 = G >> sh
    assert (zh2 <= M32).all(), "32-bit register overflow"
    r = dc.add(zh2 * dl, (F & M32) | (((G & M32) & mb) << S32))
    assert int(r.max()) < (1 << m.b) + 2 * m.delta * m.delta, "mulvv_pm result at or above 2^b + 2 delta^2"
    af, bf, rf = a.reshape(-1), b.reshape(-1), r.reshape(-1)
    for i in dc._spots(af):
        assert int(rf[i]) == mulvv_pm_int(int(af[i]), int(bf[i]), m)
    return r


def true_product_bound(q):
    """mulvv_pm's result bound in units of q: (2^b + 2 delta^2) / q"""
    m = Pm(q)
    return ((1 << m.b) + 2 * m.delta * m.delta) / q


class PmOps:
    """lazy registers of one prime; C[cid]: the constant's canonical slot values"""

    def __init__(self, m, C, reach, tag, var=None):
        self.m, self.q, self.C, self.reach, self.tag, self.var, self.underflow = m, m.q, C, reach, tag, var or {}, False

    def add(self, a, b):
        return dc.add(a, b)

    def add3(self, a, b, c):
        return dc.add(dc.add(a, b), c)

    def sub(self, a, b, off, site):
        if self.var.get("offset_too_small") == (self.tag, site):       # the wrong kernel wraps where the smaller offset does not cover b
            assert off >= 2
            t = dc.add(a, U(off // 2 * self.q))
            self.underflow = self.underflow or bool((t < b).any())
            return t - b
        return dc.sub_off(a, b, U(off * self.q))

    def mul(self, x, cid):
        self.reach.note(self.tag + " product operand", 16 * 256, x, self.q)
        r = mulvv_pm(dc.fold_pm(x, self.m), self.C[cid], self.m)
        self.reach.note(self.tag + " product", CLASSES["A"]["RQ"], r, self.q)
        return r

    def note(self, site, bound, v):
        self.reach.note("%s %s" % (self.tag, site), 16 * bound, v, self.q)


class CanOps:
    """canonical residues of all primes at once ([..., k, n]); sm: slot_craft.SlotModel; C[cid]: [k, n].  var: addmod_gt, submod_neg0"""

    def __init__(self, sm, C, var=None):
        self.sm, self.P, self.C, self.var, self.ties = sm, sm.P, C, var or {}, Counter()

    def add(self, a, b):
        s = a + b
        self.ties["sum == q"] += int((s == self.P).sum())
        self.ties["(q-1, q-1)"] += int(((a == self.P - U(1)) & (b == self.P - U(1))).sum())
        return np.where(s > self.P if self.var.get("addmod_gt") else s >= self.P, s - self.P, s)

    def add3(self, a, b, c):
        return self.add(a, self.add(b, c))

    def sub(self, a, b, off=None, site=None):
        a, b = np.broadcast_arrays(a, b)
        self.ties["difference == 0"] += int((a == b).sum())
        self.ties["0 - 0"] += int(((a == 0) & (b == 0)).sum())
        return np.where(a > b if self.var.get("submod_neg0") else a >= b, a - b, a + self.P - b)

    def mul(self, x, cid):
        return self.sm.mul(x, self.C[cid])

    def note(self, site, bound, v):
        pass


class IvOps:
    """intervals (lo, hi) in units of q; pb: the products' upper bound.  need[site] = the largest subtrahend minus the smallest minuend:
    the offset the difference needs; top[site] = the largest value at a noted site"""

    def __init__(self, pb):
        self.pb, self.need, self.off, self.top = pb, {}, {}, {}

    def add(self, a, b):
        return (a[0] + b[0], a[1] + b[1])

    def add3(self, a, b, c):
        return (a[0] + b[0] + c[0], a[1] + b[1] + c[1])

    def sub(self, a, b, off, site):
        self.need[site], self.off[site] = max(self.need.get(site, 0), b[1] - a[0]), off
        assert off >= b[1] - a[0], "%s: the offset does not cover the subtrahend" % site
        return (a[0] - b[1] + off, a[1] - b[0] + off)

    def mul(self, x, cid):
        self.note("product operand", 256, x)
        return (0, self.pb)

    def note(self, site, bound, v):
        assert v[1] <= bound, "%s: %r above %r" % (site, v[1], bound)
        self.top[site] = max(self.top.get(site, 0), v[1])


# ---- the two lines -----------------------------------------------------------------------------------------------------------------------------
def idct_line(o, d, I=1):
    """idct_line_pm<I> (offsets q IP, 16 q, 32 q) / idct_line_u64 (CanOps ignores the offsets)"""
    IP = pow2_at_least(I)
    s = o.add(d[2], d[6])
    o.note("d2+d6", 2 * I, s)
    z1 = o.mul(s, 0)
    t2, t3 = o.add(z1, o.mul(d[6], 2)), o.add(z1, o.mul(d[2], 1))
    t0, t1 = o.add(d[0], d[4]), o.sub(d[0], d[4], IP, "t1")
    t10, t13, t11, t12 = o.add(t0, t3), o.sub(t0, t3, 16, "t13"), o.add(t1, t2), o.sub(t1, t2, 16, "t12")
    u0, u1, u2, u3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = o.add(u0, u3), o.add(u1, u2), o.add(u0, u2), o.add(u1, u3)
    s = o.add(z3, z4)
    o.note("z3+z4", 4 * I, s)
    z5 = o.mul(s, 3)
    u0, u1, u2, u3 = o.mul(u0, 4), o.mul(u1, 5), o.mul(u2, 6), o.mul(u3, 7)
    z1, z2 = o.mul(z1, 8), o.mul(z2, 9)
    z3, z4 = o.add(o.mul(z3, 10), z5), o.add(o.mul(z4, 11), z5)
    u0, u1, u2, u3 = o.add3(u0, z1, z3), o.add3(u1, z2, z4), o.add3(u2, z2, z3), o.add3(u3, z1, z4)
    for u in (u0, u1, u2, u3):
        o.note("u0..u3", 24, u)
    out = [o.add(t10, u3), o.add(t11, u2), o.add(t12, u1), o.add(t13, u0),
           o.sub(t13, u0, 32, "d4"), o.sub(t12, u1, 32, "d5"), o.sub(t11, u2, 32, "d6"), o.sub(t10, u3, 32, "d7")]
    for i, v in enumerate(out):
        o.note("out sum" if i < 4 else "out difference", I + IP + (40 if i < 4 else 48), v)
    return out


IDCT_SITES = ("t1", "t13", "t12", "d4", "d5", "d6", "d7")


def dct_line(o, d, I=1):
    """dct_line_pm<I> (offsets q IP, q S1, q S2) / dct_line_u64"""
    IP, S1, S2 = pow2_at_least(I), pow2_at_least(2 * I), pow2_at_least(4 * I)
    tmp0, tmp7 = o.add(d[0], d[7]), o.sub(d[0], d[7], IP, "tmp7")
    tmp1, tmp6 = o.add(d[1], d[6]), o.sub(d[1], d[6], IP, "tmp6")
    tmp2, tmp5 = o.add(d[2], d[5]), o.sub(d[2], d[5], IP, "tmp5")
    tmp3, tmp4 = o.add(d[3], d[4]), o.sub(d[3], d[4], IP, "tmp4")
    tmp10, tmp13 = o.add(tmp0, tmp3), o.sub(tmp0, tmp3, S1, "tmp13")
    tmp11, tmp12 = o.add(tmp1, tmp2), o.sub(tmp1, tmp2, S1, "tmp12")
    d0, d4 = o.add(tmp10, tmp11), o.sub(tmp10, tmp11, S2, "d4")
    o.note("out 0", 8 * I, d0)
    o.note("out 4", 4 * I + S2, d4)
    s = o.add(tmp12, tmp13)
    o.note("tmp12+tmp13", 2 * (2 * I + S1), s)
    z1 = o.mul(s, 0)
    d2, d6 = o.add(z1, o.mul(tmp13, 1)), o.add(z1, o.mul(tmp12, 2))
    z1, z2, z3, z4 = o.add(tmp4, tmp7), o.add(tmp5, tmp6), o.add(tmp4, tmp6), o.add(tmp5, tmp7)
    s = o.add(z3, z4)
    o.note("z3+z4", 4 * (I + IP), s)
    z5 = o.mul(s, 3)
    tmp4, tmp5, tmp6, tmp7 = o.mul(tmp4, 4), o.mul(tmp5, 5), o.mul(tmp6, 6), o.mul(tmp7, 7)
    z1, z2 = o.mul(z1, 8), o.mul(z2, 9)
    z3, z4 = o.add(o.mul(z3, 10), z5), o.add(o.mul(z4, 11), z5)
    d7, d5 = o.add(o.add(tmp4, z1), z3), o.add(o.add(tmp5, z2), z4)
    d3, d1 = o.add(o.add(tmp6, z2), z3), o.add(o.add(tmp7, z1), z4)
    for v in (d2, d6):
        o.note("out 2, 6", 12, v)
    for v in (d1, d3, d5, d7):
        o.note("out odd", 24, v)
    return [d0, d1, d2, d3, d4, d5, d6, d7]


DCT_SITES = ("tmp7", "tmp6", "tmp5", "tmp4", "tmp13", "tmp12", "d4")
LINE = {"inv": (idct_line, 6, 62, IDCT_SITES), "fwd": (dct_line, 1, 24, DCT_SITES)}      # line, I of the rows, I of the columns, difference sites
TAGS = {"inv": ("idct rows", "idct cols"), "fwd": ("dct rows", "dct cols")}


def offset_table(direction, pb, structured):
    """{(pass tag, site): (offset, needed offset)} in units of q by interval arithmetic over the line.  structured = False: the source's own
    static statement -- every input of a line anywhere below I q, products below pb = 6.  structured = True: the rows' inputs are what
    they are (products for the inverse, canonical values for the forward direction), and column c is given, in all eight positions, the
    interval of the rows' output c -- the eight inputs of a column line are the SAME output of eight rows, so their offsets cancel in the
    differences.  Also returns the rows' output intervals."""
    line, I_rows, I_cols, _ = LINE[direction]
    rows, cols = IvOps(pb), IvOps(pb)
    first = (0.0, float(I_rows)) if not structured else (0.0, pb) if direction == "inv" else (0.0, 1.0)
    mid = line(rows, [first] * 8, I_rows)
    for c in range(8):
        line(cols, [mid[c] if structured else (0.0, float(I_cols))] * 8, I_cols)
    out = {(TAGS[direction][0], s): (rows.off[s], rows.need[s]) for s in rows.need}
    out.update({(TAGS[direction][1], s): (cols.off[s], cols.need[s]) for s in cols.need})
    return out, mid, rows.top, cols.top


# ---- the slot kernels of one block batch -----------------------------------------------------------------------------------------------------
def exit_pm(lazy, m, var=None):
    """canon_pm = csub(fold_pm(v), q).  -> (stored value, fold_pm's result)"""
    var = var or {}
    folded = dc.fold_pm(lazy, m)
    return (folded if var.get("exit_no_csub") else dc.csub(folded, m.q, bool(var.get("exit_gt")))), folded


def lines_pm(direction, X, i, sm, reach, var=None):
    """k_idct_lines_pm<false> + <true> / k_dct_lines_pm<false> + <true> on prime i.  X [8, 8, ..., n]: the canonical slot values the
    forward transform left, [row][col].  -> dict(final, folded, lazy [8, 8, ..., n], underflow)"""
    m, q = Pm(sm.q[i]), sm.q[i]
    line, I_rows, I_cols, _ = LINE[direction]
    C = [sm.C[c, i] for c in range(12)]
    rows_o, cols_o = PmOps(m, C, reach, TAGS[direction][0], var), PmOps(m, C, reach, TAGS[direction][1], var)
    assert (X < U(q)).all()
    mid = []
    for r in range(8):
        if direction == "inv":
            d = [mulvv_pm(dc.fold_pm(X[r, c], m), sm.inv_scale[r, c, i], m) for c in range(8)]
        else:
            d = [X[r, c] for c in range(8)]
        mid.append(line(rows_o, d, I_rows))
        for v in mid[-1]:
            rows_o.note("stored", I_cols, v)
    lazy = [[None] * 8 for _ in range(8)]
    for c in range(8):
        out = line(cols_o, [mid[r][c] for r in range(8)], I_cols)
        for r in range(8):
            lazy[r][c] = out[r] if direction == "inv" else mulvv_pm(dc.fold_pm(out[r], m), sm.fwd_scale[r, c, i], m)
    lazy = np.stack([np.stack(r) for r in lazy])
    final, folded = exit_pm(lazy, m, var)
    return dict(final=final, folded=folded, lazy=lazy, underflow=rows_o.underflow or cols_o.underflow)


def slots_canonical(direction, X, sm, var=None):
    """k_idct_slots / k_dct_slots on every prime.  X [8, 8, ..., k, n].  -> (final [8, 8, ..., k, n], ties)"""
    o = CanOps(sm, [sm.C[c] for c in range(12)], var)
    line = LINE[direction][0]
    shape = (8, 8) + (1,) * (X.ndim - 4) + (sm.k, sm.n)
    v = sm.mul(X, sm.inv_scale.reshape(shape)) if direction == "inv" else X
    mid = [line(o, [v[r, c] for c in range(8)]) for r in range(8)]
    out = [[None] * 8 for _ in range(8)]
    for c in range(8):
        res = line(o, [mid[r][c] for r in range(8)])
        for r in range(8):
            out[r][c] = res[r]
    out = np.stack([np.stack(r) for r in out])
    if direction == "fwd":
        out = sm.mul(out, sm.fwd_scale.reshape(shape))
    return out, o.ties


def run_dct(direction, blocks, sm, cls, reach=None, var=None, primes=None):
    """a batch [B, 64, 2, k, n] of coefficient-form blocks through the model of the path class `cls` takes ("A": the two-launch line
    kernels, else the one-launch slot kernel).  -> dict(final [B, 64, 2, k, n] slot values, per-prime pm results or the ties)"""
    S = np.stack([sm.to_slots(b) for b in blocks])                              # [B, 8, 8, 2, k, n]
    X = np.moveaxis(S, 0, 2)                                                    # [8, 8, B, 2, k, n]
    if cls != "A":
        final, ties = slots_canonical(direction, X, sm, var)
        return dict(final=np.moveaxis(final, 2, 0).reshape(blocks.shape), ties=ties)
    reach = Reach() if reach is None else reach
    final, pm = np.empty_like(X), {}
    for i in (range(sm.k) if primes is None else primes):
        pm[i] = lines_pm(direction, np.ascontiguousarray(X[..., i, :]), i, sm, reach, var)
        final[..., i, :] = pm[i]["final"]
    return dict(final=np.moveaxis(final, 2, 0).reshape(blocks.shape), pm=pm, reach=reach)


def to_coeffs(sm, slots):
    """[..., k, n] slot values -> coefficients (the oracle's inverse transform)"""
    out = np.empty_like(slots)
    for idx in np.ndindex(slots.shape[:-2]):
        for i in range(sm.k):
            out[idx][i] = sm.orc.ntt_inv(slots[idx][i], i)
    return out


def to_slots(sm, coeffs):
    out = np.empty_like(coeffs)
    for idx in np.ndindex(coeffs.shape[:-2]):
        for i in range(sm.k):
            out[idx][i] = sm.orc.ntt_fwd(coeffs[idx][i], i)
    return out


# ---- families of the two DCT directions ---------------------------------------------------------------------------------------------------------
def delta_of(q):
    return min((1 << q.bit_length()) - q, 1 << 31)


_PAIRS = {}


def first_stage_pairs(sm, i):
    """(a, b): the slots, in the oracle's order, that the network holds at positions 2j and 2j + 1 -- the operands X and Y of the first
    butterflies an inverse transform runs (stage L - 1: the two evaluation points w and -w)"""
    key = (sm.q[i], sm.n)
    if key not in _PAIRS:
        mono = np.zeros(sm.n, dtype=U)
        mono[1] = 1
        perm = nc.slot_permutation(nc.exact_fwd([0, 1] + [0] * (sm.n - 2), nc.tables(sm.q[i], sm.n)), sm.orc.ntt_fwd(mono, i))
        _PAIRS[key] = (perm[0::2], perm[1::2])
    return _PAIRS[key]


def transform_entry_wraps(stored, sm, i):
    """What the API can see of a line kernel's exit.  k_ntt_inv_pm takes the stored words as canonical (entry bound q) and opens with
    D = X - Y + q: a stored q + r (exit without its subtraction) is congruent and harmless unless its partner X is below r -- then D wraps
    modulo 2^64.  A stored q itself (`>` for `>=`) never wraps.  stored [..., n] of prime i -> the number of first butterflies that wrap"""
    a, b = first_stage_pairs(sm, i)
    return int((stored[..., a] + U(sm.q[i]) < stored[..., b]).sum())


def e_targets(sm, seed=SEED):
    """[8, 8, 2, k, n] prescribed output residues.  Slots with (slot + output + polynomial) even draw from 0, 1, delta - 1 and random values
    below delta; the others from delta, q - delta, q - 1 and random values at or above delta.  One first-stage pair in eight is given to the
    transform behind the kernel: at one of its slots ALL 64 outputs are 0 -- so are the inputs, and output (0, 0), the one lazy value
    without an offset, is 0 itself -- and at the other output (0, 0) is 1 .. delta - 1 under its lazy sum: X = 0 beside Y = q + r if the exit
    forgets its subtraction.  Both orientations, alternating, so that the test does not depend on which slot the kernel calls X."""
    out = np.empty((8, 8, 2, sm.k, sm.n), dtype=U)
    idx = np.arange(64).reshape(8, 8, 1, 1) + np.arange(2).reshape(1, 1, 2, 1) + np.arange(sm.n).reshape(1, 1, 1, sm.n)
    for i, q in enumerate(sm.q):
        rng, dl = np.random.default_rng([seed, sm.n, i]), delta_of(q)
        pick = rng.integers(0, 4, size=idx.shape)
        low = np.choose(pick, [0, 1, dl - 1, rng.integers(0, dl, size=idx.shape)])
        high = np.choose(pick, [dl, q - dl, q - 1, dl + rng.integers(0, q - dl, size=idx.shape)])
        out[:, :, :, i, :] = np.where(idx % 2 == 0, low, high).astype(U)
        a, b = first_stage_pairs(sm, i)
        j = np.arange(sm.n // 2)
        for zero, small in ((a[j % 16 == 0], b[j % 16 == 0]), (b[j % 16 == 8], a[j % 16 == 8])):
            out[:, :, :, i, zero] = 0
            for p in range(2):
                out[0, 0, p, i, small] = (1 + np.arange(len(small)) % max(dl - 1, 1)).astype(U)
    return out


def block_from_slots(sm, X, ok, rng):
    """X [8, 8, 2, k, n] slot values, ok [2, k, n] -> coefficient block [64, 2, k, n]; left-out slots get random values and are counted"""
    bad = int((~ok).sum())
    sm.left_out += bad
    sm.crafted += ok.size
    assert bad <= sc.MAX_LEFT_OUT * ok.size, "the solver left out %d of %d slots" % (bad, ok.size)
    if bad:
        X = np.where(ok, X, rng.integers(0, 1 << 62, size=X.shape, dtype=np.int64).astype(U) % sm.P)
    return to_coeffs(sm, X.reshape(64, 2, sm.k, sm.n))


def craft_e(sm, direction, seed=SEED):
    """-> (block, targets [8, 8, 2, k, n], solved mask [2, k, n])"""
    G = e_targets(sm, seed + (direction == "fwd"))
    craft = sm.craft_inv_f4 if direction == "inv" else sm.craft_fwd_f4
    sol = [craft(np.ascontiguousarray(G[:, :, p])) for p in range(2)]
    X, ok = np.stack([s[0] for s in sol], axis=2), np.stack([s[1] for s in sol])
    return block_from_slots(sm, X, ok, np.random.default_rng(seed)), G, ok


Z_NAMES = ("zero", "one", "top", "half-", "half+")


def z_value(q, name):
    return {"zero": 0, "one": 1, "top": q - 1, "half-": (q - 1) // 2, "half+": (q + 1) // 2}[name]


def craft_batch(sm, direction, seed=SEED):
    """-> (names, blocks [B, 64, 2, k, n], E targets, E mask).  Families Z, E, T (slot_craft's F1, the F2 ties, F3) and one random block"""
    rng = np.random.default_rng(seed)
    blocks = [("Z-" + nm, sm.constant_block([[z_value(p, nm) for p in sm.q]] * 64)) for nm in Z_NAMES]
    eb, G, ok = craft_e(sm, direction, seed)
    blocks.append(("E", eb))
    blocks.append(("T-ties", sm.constant_block(sm.f2_constants()["ties"])))
    if direction == "fwd":
        blocks += [("T-F1", sm.block(sm.craft_fwd_f1(), rng)), ("T-F3", sm.block(sm.craft_fwd_f3(), rng))]
    else:
        blocks += [("T-F1", sm.block(sm.craft_inv_f1(), rng)), ("T-F3", sm.block(sm.craft_inv_f3(+1), rng)), ("T-F3-diff", sm.block(sm.craft_inv_f3(-1), rng))]
    blocks.append(("random", sm.orc.random_ct(64, seed=seed)))
    assert len(blocks) <= 12
    return [a for a, _ in blocks], np.stack([b for _, b in blocks]), G, ok


def exit_counts(res, sm):
    """per prime: (outputs where csub is taken, where it is not, where fold_pm's result is exactly q) over a pm result of run_dct"""
    return {i: (int((r["folded"] >= U(sm.q[i])).sum()), int((r["folded"] < U(sm.q[i])).sum()), int((r["folded"] == U(sm.q[i])).sum()))
            for i, r in res["pm"].items()}


# ---- colour ---------------------------------------------------------------------------------------------------------------------------------------
class Colour:
    """the constants of both conversions at the slots and Delta encode(128) of one SlotModel"""

    def __init__(self, sm):
        self.sm = sm
        orc = sm.orc
        self.rgb = [sm.plain_slots(orc.encode(v)) for v in RGB_CONSTS]          # 9 x [k, n]
        self.ycc = [sm.plain_slots(orc.encode(v)) for v in YCC_CONSTS]          # 4 x [k, n]
        self.off = orc.add_plain(np.zeros((2, sm.k, sm.n), dtype=U), orc.encode(128.0))[0]      # [k, n]: polynomial 0 of 0 + encode(128)
        self.off_at = sorted(set(np.nonzero(self.off)[1].tolist()))
        assert len(self.off_at) == 1, "Delta encode(128) has one non-zero coefficient"
        self.J = self.off_at[0]
        self.offv = [int(self.off[i, self.J]) for i in range(sm.k)]


def prescribed_pixels(n):
    """16 crafted pixels at n = 1024; at n = 8192 four, the fewest with which each polynomial meets all four words at coefficient J"""
    return 16 if n == N else 4


def _offset(o, y, off, var, sign):
    """the offset on polynomial 0 (and, wrongly, on polynomial 1; or with the wrong sign).  y [P, 2, k, n]"""
    add = (sign > 0) != bool(var.get("offset_sign"))
    out = y.copy()
    for p in ((0, 1) if var.get("offset_on_poly1") else (0,)):
        out[:, p] = o.add(y[:, p], off) if add else o.sub(y[:, p], off)
    return out


def ycc2rgb_canonical(col, ycc, var=None):
    """k_ycc2rgb as residue arithmetic.  ycc [3, P, 2, k, n] coefficients -> (rgb [3, P, 2, k, n], ties)"""
    var, sm = var or {}, col.sm
    o = CanOps(sm, col.ycc, var)
    cb, cr = to_slots(sm, ycc[1]), to_slots(sm, ycc[2])
    r = o.mul(cr, 0)
    g = o.sub(o.sub(np.zeros_like(cb), o.mul(cb, 1)), o.mul(cr, 2))
    b = o.mul(cb, 3)
    stored_q = int((g >= sm.P).sum())                                             # a wrong submod leaves q itself in a register
    r, g, b = (to_coeffs(sm, x % sm.P) for x in (r, g, b))
    yy = _offset(o, ycc[0], col.off, var, +1)
    out = np.stack([o.add(yy, r), o.add(yy, g), o.add(yy, b)])
    o.ties["q in a register"] = stored_q
    return out, o.ties


def rgb2ycc_canonical(col, rgb, var=None):
    """k_rgb2ycc as residue arithmetic.  rgb [3, P, 2, k, n] -> (ycc, ties)"""
    var, sm = var or {}, col.sm
    o = CanOps(sm, col.rgb, var)
    r, g, b = (to_slots(sm, x) for x in rgb)
    y = o.add(o.add(o.mul(r, 0), o.mul(g, 1)), o.mul(b, 2))
    u = o.add(o.sub(o.mul(r, 3), o.mul(g, 4)), o.mul(b, 5))
    v = o.sub(o.sub(o.mul(r, 6), o.mul(g, 7)), o.mul(b, 8))
    y, u, v = (to_coeffs(sm, x % sm.P) for x in (y, u, v))
    return np.stack([_offset(o, y, col.off, var, -1), u, v]), o.ties


def rgb_sum_bound(rq):
    return rq + 2 * (16 << nc.clog(rq))


def rgb_pm_unit(col, rgb_unit, i, poly, cls, reach, var=None):
    """k_rgb_ntt_pm<L, C, false>, k_rgb_combine_pm<C>, k_rgb_ntt_pm<L, C, true> on one (pixel, polynomial, prime): rgb_unit [3, n]
    coefficients.  -> dict(final [3, n], folded, lazy, underflow).  Sites record sixteenths of q."""
    var, sm = var or {}, col.sm
    q, n, c = sm.q[i], sm.n, CLASSES[cls]
    T, m = nc.tables(q, n), Pm(q)
    mono = np.zeros(n, dtype=U)
    mono[1] = 1
    perm = nc.slot_permutation(nc.exact_fwd([0, 1] + [0] * (n - 2), T), sm.orc.ntt_fwd(mono, i))
    K = [col.rgb[cid][i][perm] for cid in range(9)]
    fwd = np.array([nc.pm_forward_lazy(x, T, cls, []) for x in rgb_unit], dtype=U)
    reach.note("rgb forward out (class %s)" % cls, nc.pm_fwd_bound(16, c["LIM"], c["CS"], T.L), fwd, q, strict=False)
    assert int(fwd.max()) < 1 << 62
    rr, gg, bb = (dc.fold_pm(x, m) for x in fwd)
    M = lambda x, cid: mulvv_pm(x, K[cid], m)
    prods = [M(rr, 0), M(gg, 1), M(bb, 2), M(rr, 3), M(gg, 4), M(bb, 5), M(rr, 6), M(gg, 7), M(bb, 8)]
    for p in prods:
        reach.note("rgb product (class %s)" % cls, c["RQ"], p, q, strict=False)
    sh = nc.clog(c["RQ"])
    small, underflow = var.get("offset_too_small") == ("rgb combine", "off"), False

    def neg(p):
        nonlocal underflow
        off = U(q << (sh - 1 if small else sh))
        underflow = underflow or bool((off < p).any())
        return off - p if small else dc.sub_off(off, p, U(0))

    y = dc.add(dc.add(prods[0], prods[1]), prods[2])
    u = dc.add(dc.add(prods[3], prods[5]), neg(prods[4]))
    v = dc.add(dc.add(prods[6], neg(prods[7])), neg(prods[8]))
    e0 = rgb_sum_bound(c["RQ"])
    lazy = []
    for plane in (y, u, v):
        reach.note("rgb sum (class %s)" % cls, e0, plane, q, strict=False)
        if small and underflow:                                  # a wrapped value is outside what the inverse transform's plan admits
            lazy.append([int(x) for x in plane])
            continue
        lazy.append(nc.pm_inverse_lazy([int(x) for x in plane], T, cls, [], e0=e0))
    lazy = np.array(lazy, dtype=U)
    final, folded = exit_pm(lazy, m, var)
    if poly == 0 or var.get("offset_on_poly1"):
        offc, Pq = col.off[i], U(q)
        if var.get("offset_sign"):
            s = final[0] + offc
            final[0] = np.where(s >= Pq, s - Pq, s)
        else:
            final[0] = np.where(final[0] > offc if var.get("submod_neg0") else final[0] >= offc, final[0] - offc, final[0] + Pq - offc)
    return dict(final=final, folded=folded, lazy=lazy, underflow=underflow)


def _ring_div(sm, coeffs, const):
    """the polynomial whose product with the constant (slot values const [k, n]) is `coeffs` [..., k, n]; slots where the constant is
    zero are left zero and counted"""
    inv, nz = sm.inv(const)
    sm.left_out += int((~nz).sum())
    sm.crafted += nz.size
    assert int((~nz).sum()) <= sc.MAX_LEFT_OUT * nz.size
    return to_coeffs(sm, sm.mul(to_slots(sm, coeffs), inv))


def _cycle(words, shape_n, shift):
    """[k, n]: coefficient j of prime i holds words[i][(j + shift) % len]"""
    j = (np.arange(shape_n) + shift) % len(words[0])
    return np.stack([np.array(w, dtype=object)[j].astype(U) for w in words])


def craft_ycc(col, prescribed, seed=SEED):
    """one colour block [3 (Y, Cb, Cr), 64, 2, k, n] for ycc_to_rgb.  Pixels below `prescribed`: the products Cr 1.402 and Cb 1.772 are
    prescribed coefficient by coefficient and Y is chosen so that the last addmod meets exactly q, q - 1, 0 + 0 and (q-1) + (q-1); at
    coefficient J (where Delta encode(128) is not zero) both polynomials of Y hold 0, q - 1, q - off and q - off - 1.  The next eight
    pixels have Cb = Cr = 0 (submod(0, 0) at every slot) under the same Y words; the rest are random (n = 1024) or zero."""
    sm = col.sm
    q, k, n, rng = sm.q, sm.k, sm.n, np.random.default_rng([seed, sm.n])
    blk = np.zeros((3, 64, 2, k, n), dtype=U)
    if n == N:
        blk[:, prescribed + 8:] = sm.orc.random_ct(3 * 64, seed=seed).reshape(3, 64, 2, k, n)[:, prescribed + 8:]
    rnd = [[int(x) for x in rng.integers(1, p - 1, size=4)] for p in q]
    # (product word, word of Y + offset) pairs: sums 0, q, q, 2q - 2, q - 1, q - 1, q, q, q - 1
    pairs = [[(0, 0), (1, p - 1), (p - 1, 1), (p - 1, p - 1), (0, p - 1), (p - 1, 0), ((p - 1) // 2, (p + 1) // 2), (r[0], p - r[0]), (r[1], p - 1 - r[1])]
             for p, r in zip(q, rnd)]
    yj = [[0, p - 1, p - o, p - o - 1] for p, o in zip(q, col.offv)]
    Pr, Pb = np.zeros((64, 2, k, n), dtype=U), np.zeros((64, 2, k, n), dtype=U)
    for px in range(prescribed + 8):
        for s in range(2):
            pr = _cycle([[a for a, _ in w] for w in pairs], n, px + s)
            yy = _cycle([[b for _, b in w] for w in pairs], n, px + s)
            y = yy.copy()
            y[:, col.J] = [yj[i][(px + s) % 4] for i in range(k)]               # the same words in both polynomials
            yyJ = (y[:, col.J] + (col.off[:, col.J] if s == 0 else U(0))) % sm.P[:, 0]
            yy[:, col.J] = yyJ
            # the B product against the same Y': sums q (or 0 + 0), q - 1, Y' alone, Y' + (q - 1), by coefficient
            sel = ((np.arange(n) // len(pairs[0])) + px) % 4
            pb = np.where(sel == 0, (sm.P - yy) % sm.P, np.where(sel == 1, (sm.P - U(1) - yy) % sm.P, np.where(sel == 2, U(0), sm.P - U(1))))
            blk[0, px, s] = y
            if px < prescribed:
                Pr[px, s], Pb[px, s] = pr, pb
    blk[2, :prescribed] = _ring_div(sm, Pr[:prescribed], col.ycc[0])
    blk[1, :prescribed] = _ring_div(sm, Pb[:prescribed], col.ycc[3])
    return blk, Pr, Pb


def craft_rgb(col, prescribed, seed=SEED):
    """one colour block [3 (R, G, B), 64, 2, k, n] for rgb_to_ycc.  Pixels below `prescribed`: the three outputs in front of the offset are
    prescribed coefficient by coefficient (the exits' words of family E, 0 and q - 1) and the 3 x 3 system is solved per slot; at
    coefficient J both polynomials of Y hold 0, q - 1, off and off - 1 in front of the subtraction.  The next two pixels put ties under
    the one-launch kernel's slot arithmetic: G = -(R 0.299) / 0.587 with B = 0 (the first addmod of y meets exactly q at every slot where
    the product is not zero) and G = R (-0.168736) / 0.331264 (the submod of u meets two equal operands).  A third has R = B = 0 and the product
    G 0.331264 prescribed AT THE SLOTS to 1 .. delta - 1: mulvv_pm returns q + r there, the largest subtrahend k_rgb_combine_pm's
    off - M(gg, 4) meets (a class-B offset of q instead of 2 q would wrap).  Then five all-zero pixels; the rest random (n = 1024) or zero.  -> (block, prescribed outputs [3, prescribed, 2, k, n] in front of the offset, solved mask)"""
    sm = col.sm
    q, k, n = sm.q, sm.k, sm.n
    blk = np.zeros((3, 64, 2, k, n), dtype=U)
    if n == N:
        blk[:, prescribed + 8:] = sm.orc.random_ct(3 * 64, seed=seed + 1).reshape(3, 64, 2, k, n)[:, prescribed + 8:]
    want = np.empty((3, prescribed, 2, k, n), dtype=U)
    for i, p in enumerate(q):
        rng, dl = np.random.default_rng([seed, n, i, 7]), delta_of(p)
        shape = (3, prescribed, 2, n)
        idx = np.arange(3).reshape(3, 1, 1, 1) + np.arange(prescribed).reshape(1, -1, 1, 1) + np.arange(2).reshape(1, 1, 2, 1) + np.arange(n).reshape(1, 1, 1, n)
        pick = rng.integers(0, 4, size=shape)
        low = np.choose(pick, [0, 1, dl - 1, rng.integers(0, dl, size=shape)])
        high = np.choose(pick, [dl, p - dl, p - 1, dl + rng.integers(0, p - dl, size=shape)])
        want[:, :, :, i, :] = np.where(idx % 2 == 0, low, high).astype(U)
        yj = [0, p - 1, col.offv[i], col.offv[i] - 1]
        for px in range(prescribed):
            for s in range(2):
                want[0, px, s, i, col.J] = yj[(px + s) % 4]
    A = np.stack([np.stack([col.rgb[3 * r + c] if (r, c) not in ((1, 1), (2, 1), (2, 2)) else sm.neg(col.rgb[3 * r + c]) for c in range(3)]) for r in range(3)])
    W = to_slots(sm, want)
    sol, ok = sm.solve(A, W.reshape(3, prescribed * 2, k, n))
    bad = int((~ok).sum())
    sm.left_out += bad
    sm.crafted += ok.size
    assert bad <= sc.MAX_LEFT_OUT * ok.size
    sol = np.where(ok, sol, U(0))
    blk[:, :prescribed] = to_coeffs(sm, sol.reshape(3, prescribed, 2, k, n))
    R = to_slots(sm, sm.orc.random_ct(2, seed=seed + 2))                           # [2, 2, k, n]
    for px, (num, den, negate) in enumerate(((0, 1, True), (3, 4, False))):
        inv, nz = sm.inv(col.rgb[den])
        g = sm.mul(sm.mul(R[px], col.rgb[num]), inv)
        blk[0, prescribed + px], blk[1, prescribed + px] = to_coeffs(sm, R[px]), to_coeffs(sm, np.where(nz, sm.neg(g) if negate else g, U(0)))
    small = np.stack([U(1) + (np.arange(n, dtype=U) % U(max(delta_of(p) - 1, 1))) for p in q])      # [k, n]: 1 .. delta - 1
    inv, nz = sm.inv(col.rgb[4])
    blk[1, prescribed + 2] = to_coeffs(sm, np.broadcast_to(np.where(nz, sm.mul(small, inv), U(0)), (2, k, n)).copy())
    return blk, want, ok
