"""An exact integer model of the fused FP64 DCT / IDCT pair (csrc/dct_fused.hip) at the NTT slots, and inputs crafted
with it that put chosen residues under the kernels' products and reductions.

Everything here is integer arithmetic modulo each prime; no floating point is involved.  Residues are numpy uint64
arrays shaped [..., k, n] (n slots in the CPU oracle's NTT order), centred values and sums of centred values are int64.
A modular product of two residues is formed from limbs of 63 - bits(p) bits so that no intermediate leaves 64 bits, for
primes of up to 57 bits (test_slot_craft_cpu.py checks it against Python integers up to 48 bits, test_dct_u64_craft_cpu.py
up to 57); from 58 to 61 bits the product runs on Python integers (jpeg_u64_craft.py's 58- and 61-bit bases).

The model is slotwise, so the order in which the kernels hold the slots does not matter: a constant's slot value meets
the data's value of the same slot in every order.

What a product "sees".  mm(y, w) (csrc/fp64_core.h) returns the centred remainder of y * w, which depends on the residue
of y only; sums of such remainders are formed without reduction.  The model therefore reproduces exactly
  forward rows:  the stored outputs 1/3/5/7 (four centred products), 2/6 (two) and, in the packed variant, 0/4 (reduced)
  forward cols:  the operand of every scale product for outputs 1/3/5/7 and 2/6, and all final residues
  inverse rows:  the scaled inputs, every product, E and O before their reduction and as stored
  inverse cols:  the eight inputs E +- O, every product operand (z3 + z4 among them), and all final residues
and does NOT reproduce magnitudes that depend on the unreduced transforms (the forward rows' inputs, the inverse
transform's running sums); for those the crafted inputs fix the residues and the bound follows from n and p.

Each line is written in "half variables", the way the kernels split it:
  forward line  d0..d7 -> a = (tmp0..tmp3) = d_m + d_(7-m),  b = (tmp4..tmp7) with tmp_(7-m) = d_m - d_(7-m);
                the even half maps a to outputs 0 2 4 6, the odd half b to outputs 1 3 5 7
  inverse line  a = (d0 d2 d4 d6) -> E0..E3,  b = (d1 d3 d5 d7) -> O0..O3;  out[m] = E[m] + O[m], out[7-m] = E[m] - O[m]
so every system that is solved is 4 x 4 per slot (Gauss-Jordan modulo p with a per-slot pivot search)."""
import numpy as np

from idct_oracle import IDCT_CONSTS as LINE_CONSTS      # the twelve LL&M constants, shared by both directions

U = np.uint64

# ---------------------------------------------------------------------------------------------------------------------
# contexts of tests/test_gpu_dct_slot_extremes.py (also walked by the CPU file)
# ---------------------------------------------------------------------------------------------------------------------
T = 1 << 14
Q36 = [0xFFFF00001, 0xFFFE58001, 0xFFFCB8001]              # <= 37 bits: packed intermediate
P4096 = [0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001]           # the headline primes; the last one has 37 bits
Q40 = [0xFFFFE80001, 0x7FFFFB0001, 0x7FFFE60001]           # 39/40 bits: FP64 intermediate
Q46 = [0x3FFFFFF70001, 0x7FFFFFFC8001, 0xFFFFFDF8001]      # 44..47 bits: BIG
# Primes p = 1 (mod 2^14) next to each threshold of the variant choice, found with search_prime() below (Miller-Rabin
# over the fixed bases that are a proof below 3.3e24); test_slot_craft_cpu.py repeats the search.
P_ABOVE_37 = 0x2000088001        # search_prime(2^37, +1): smallest above 2^37 -- must leave the packed variant
P_ABOVE_40 = 0x10000048001       # search_prime(2^40, +1): smallest above 2^40 -- must take BIG
P_BELOW_47 = 0x7FFFFFFEC001      # search_prime(2^47, -1): largest below 2^47 -- the last prime the fused pair accepts
P_ABOVE_47 = 0x800000020001      # search_prime(2^47, +1): smallest above 2^47 -- must leave the fused pair
THRESHOLD_SETS = {
    "above37": [P_ABOVE_37, Q36[0], Q36[1]],
    "above40": [P_ABOVE_40, Q40[0], Q40[1]],
    "below47": [P_BELOW_47, Q46[0], Q46[2]],
    "above47": [P_ABOVE_47, Q46[0], Q46[2]],
}


# name -> (n, primes, switches, the fused FP64 pair is expected to run).  Four sizes x three prime classes reach every
# launch_pair / launch_ipair case; the switch variants reach the bodies that no default context takes; the threshold sets
# sit right next to each change of variant.
GPU_CONTEXTS = {}
for _n in (1024, 2048, 4096, 8192):
    GPU_CONTEXTS["n%d-36b" % _n if _n != 4096 else "P4096"] = (_n, Q36 if _n != 4096 else P4096, {}, True)
    GPU_CONTEXTS["n%d-40b" % _n] = (_n, Q40, {}, True)
    GPU_CONTEXTS["n%d-46b" % _n] = (_n, Q46, {}, True)
GPU_CONTEXTS.update({
    "P4096-pack0": (4096, P4096, {"FHE_DCT_PACK": 0}, True),
    "P4096-ldsc0": (4096, P4096, {"FHE_DCT_LDSC": 0}, True),
    "P4096-le4": (4096, P4096, {"FHE_DCT_LE": 4}, True),
    "n8192-36b-le4": (8192, Q36, {"FHE_DCT_LE": 4}, True),
    "n8192-46b-le4": (8192, Q46, {"FHE_DCT_LE": 4}, True),
})
for _n in (4096, 8192):
    for _name, _q in THRESHOLD_SETS.items():
        GPU_CONTEXTS["n%d-%s" % (_n, _name)] = (_n, _q, {}, _name != "above47")


def is_prime(m):
    if m < 2:
        return False
    bases = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for b in bases:
        if m % b == 0:
            return m == b
    d, s = m - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for b in bases:
        x = pow(b, d, m)
        if x in (1, m - 1):
            continue
        for _ in range(s - 1):
            x = x * x % m
            if x == m - 1:
                break
        else:
            return False
    return True


def search_prime(bound, direction, step=1 << 14):
    """the prime p = 1 (mod step) nearest to `bound` (a multiple of step) above it (+1) or below it (-1)"""
    p = bound + 1 if direction > 0 else bound - step + 1
    while not is_prime(p):
        p += step if direction > 0 else -step
    return p


# ---------------------------------------------------------------------------------------------------------------------
# the two lines in half variables: products name -> (constant id, coefficients), plain sums, outputs as signed terms
# ---------------------------------------------------------------------------------------------------------------------
class Half:
    def __init__(self, prod, plain, out):
        self.prod, self.plain, self.out = prod, plain, out


# fp64::line_half<0>: a = (tmp0 tmp1 tmp2 tmp3); tmp12 + tmp13 = a0 + a1 - a2 - a3, tmp13 = a0 - a3, tmp12 = a1 - a2
FWD_EVEN = Half({"e0": (0, (1, 1, -1, -1)), "e1": (1, (1, 0, 0, -1)), "e2": (2, (0, 1, -1, 0))},
                {"s0": (1, 1, 1, 1), "s4": (1, -1, -1, 1)},
                {0: [(1, "s0")], 2: [(1, "e0"), (1, "e1")], 4: [(1, "s4")], 6: [(1, "e0"), (1, "e2")]})
# fp64::line_half<1>: b = (tmp4 tmp5 tmp6 tmp7); z1 = tmp4 + tmp7, z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7
FWD_ODD = Half({"z5": (3, (1, 1, 1, 1)), "t4": (4, (1, 0, 0, 0)), "t5": (5, (0, 1, 0, 0)), "t6": (6, (0, 0, 1, 0)),
                "t7": (7, (0, 0, 0, 1)), "z1": (8, (1, 0, 0, 1)), "z2": (9, (0, 1, 1, 0)), "z3": (10, (1, 0, 1, 0)),
                "z4": (11, (0, 1, 0, 1))}, {},
               {1: [(1, "t7"), (1, "z1"), (1, "z4"), (1, "z5")], 3: [(1, "t6"), (1, "z2"), (1, "z3"), (1, "z5")],
                5: [(1, "t5"), (1, "z2"), (1, "z4"), (1, "z5")], 7: [(1, "t4"), (1, "z1"), (1, "z3"), (1, "z5")]})
# idct_half<0>: a = (d0 d2 d4 d6); outputs E0..E3 = t0 + t3, t1 + t2, t1 - t2, t0 - t3 with t2 = e0 + e1, t3 = e0 + e2
INV_EVEN = Half({"e0": (0, (0, 1, 0, 1)), "e1": (2, (0, 0, 0, 1)), "e2": (1, (0, 1, 0, 0))},
                {"t0": (1, 0, 1, 0), "t1": (1, 0, -1, 0), "d0": (1, 0, 0, 0), "d4": (0, 0, 1, 0)},
                {0: [(1, "t0"), (1, "e0"), (1, "e2")], 1: [(1, "t1"), (1, "e0"), (1, "e1")],
                 2: [(1, "t1"), (-1, "e0"), (-1, "e1")], 3: [(1, "t0"), (-1, "e0"), (-1, "e2")]})
# idct_half<1>: b = (d1 d3 d5 d7) = (u3 u2 u1 u0); z1 = u0 + u3, z2 = u1 + u2, z3 = u0 + u2, z4 = u1 + u3; outputs O0..O3
INV_ODD = Half({"z5": (3, (1, 1, 1, 1)), "u0": (4, (0, 0, 0, 1)), "u1": (5, (0, 0, 1, 0)), "u2": (6, (0, 1, 0, 0)),
                "u3": (7, (1, 0, 0, 0)), "z1": (8, (1, 0, 0, 1)), "z2": (9, (0, 1, 1, 0)), "z3": (10, (0, 1, 0, 1)),
                "z4": (11, (1, 0, 1, 0))}, {},
               {0: [(1, "u3"), (1, "z1"), (1, "z4"), (1, "z5")], 1: [(1, "u2"), (1, "z2"), (1, "z3"), (1, "z5")],
                2: [(1, "u1"), (1, "z2"), (1, "z4"), (1, "z5")], 3: [(1, "u0"), (1, "z1"), (1, "z3"), (1, "z5")]})
FWD_ODD_OUTPUTS = (1, 3, 5, 7)
MAX_LEFT_OUT = 0.01          # a crafted block is valid only if at most this share of its slots could not be solved


class SlotModel:
    def __init__(self, orc, quant):
        self.orc, self.n, self.k, self.q = orc, orc.n, orc.k, list(orc.q)
        self.P = np.array(self.q, dtype=U).reshape(self.k, 1)
        self.Pi = self.P.astype(np.int64)
        self.H = (self.P - U(1)) // U(2)                            # (p - 1) / 2: the largest centred residue
        bits = max(p.bit_length() for p in self.q)
        assert bits <= 61                                           # the library's own limit; above 57 bits mul() runs on Python integers
        self.w = 63 - bits if bits <= 57 else 0                     # limbs of at least 6 bits (dct_u64_craft.py: the fused u64 pair's primes)
        self.limbs = -(-bits // self.w) if self.w else 0
        self.inv2 = (self.P + U(1)) // U(2)
        self.C = np.stack([self.plain_slots(orc.encode(v)) for v in LINE_CONSTS])                # [12, k, n]
        e8 = self.plain_slots(orc.encode(0.125))
        # forward: encode(0.125) then encode(1 / Q[i]) on output i; inverse: encode(Q[i]) * encode(0.125) on input i
        self.fwd_scale = np.stack([self.mul(e8, self.plain_slots(orc.encode(1 / float(v)))) for v in quant]).reshape(8, 8, self.k, self.n)
        self.inv_scale = np.stack([self.mul(self.plain_slots(orc.encode(float(v))), e8) for v in quant]).reshape(8, 8, self.k, self.n)
        self.left_out = 0                                          # slots left out by the solver, summed over what was crafted
        self.crafted = 0                                           # slots the solver was asked for
        self._inv_cache = {}

    # -- arithmetic -----------------------------------------------------------------------------------------------
    def plain_slots(self, plain):
        lift = self.orc.plain_lift(plain)
        return np.stack([self.orc.ntt_fwd(lift[i], i) for i in range(self.k)])

    def mul(self, a, b):
        if not self.w:                                              # 58..61 bits (jpeg_u64_craft.py): no limb width leaves room in 64 bits
            return (np.asarray(a).astype(object) * np.asarray(b).astype(object) % self.P.astype(object)).astype(U)
        mask, w, r = U((1 << self.w) - 1), U(self.w), None
        for i in reversed(range(self.limbs)):
            t = a * ((b >> U(self.w * i)) & mask)
            r = t % self.P if r is None else ((r << w) + t) % self.P
        return r

    def add(self, a, b):
        return (a + b) % self.P

    def sub(self, a, b):
        return (a + (self.P - b)) % self.P

    def neg(self, a):
        return (self.P - a) % self.P

    def centre(self, a):
        s = a.astype(np.int64)
        return np.where(a > self.H, s - self.Pi, s)

    def res(self, v):
        """int64 values -> residues"""
        return np.mod(v, self.Pi).astype(U)

    def full(self, v):
        """a residue per prime (list of Python integers, or one integer) -> [k, n]"""
        v = [v] * self.k if isinstance(v, int) else v
        return np.broadcast_to(np.array([x % p for x, p in zip(v, self.q)], dtype=U).reshape(self.k, 1), (self.k, self.n)).copy()

    def inv(self, a):
        """slotwise modular inverse by a product tree along the slots and one Python pow per tree; (inverse, nonzero mask)"""
        nz = a != 0
        levels = [np.where(nz, a, U(1))]
        while levels[-1].shape[-1] > 1:
            t = levels[-1]
            levels.append(self.mul(t[..., 0::2], t[..., 1::2]))
        root = levels[-1]
        r = np.empty_like(root)
        for idx in np.ndindex(root.shape):
            r[idx] = pow(int(root[idx]), -1, self.q[idx[-2]])
        for t in reversed(levels[:-1]):
            nxt = np.empty_like(t)
            nxt[..., 0::2] = self.mul(r, t[..., 1::2])
            nxt[..., 1::2] = self.mul(r, t[..., 0::2])
            r = nxt
        return np.where(nz, r, U(0)), nz

    def solve(self, A, Tg):
        """A [m, m, k, n], Tg [m, r, k, n] -> (X [m, r, k, n] with A X = Tg per slot, solvable mask [k, n])"""
        A, Tg, m = A.copy(), Tg.copy(), A.shape[0]
        ok = np.ones(A.shape[2:], dtype=bool)
        for j in range(m):
            nzc = A[j:, j] != 0
            idx = nzc.argmax(0) + j
            ok &= nzc.any(0)
            for M in (A, Tg):                                       # per slot: swap row j with the pivot row
                g = np.broadcast_to(idx, M.shape[1:])[None]
                rowj = M[j].copy()
                M[j] = np.take_along_axis(M, g, 0)[0]
                np.put_along_axis(M, g, rowj[None], 0)
            piv, _ = self.inv(A[j, j])
            A[j], Tg[j] = self.mul(A[j], piv), self.mul(Tg[j], piv)
            for i in range(m):
                if i != j:
                    f = A[i, j].copy()
                    A[i], Tg[i] = self.sub(A[i], self.mul(f, A[j])), self.sub(Tg[i], self.mul(f, Tg[j]))
        return Tg, ok

    # -- functionals ----------------------------------------------------------------------------------------------
    def coef(self, half, terms):
        """coefficients [4, k, n] of sum(sign * term) over the half's four variables; a term is a product or a plain sum"""
        row = np.zeros((4, self.k, self.n), dtype=U)
        for sign, name in terms:
            cid, vec = half.prod[name] if name in half.prod else (None, half.plain[name])
            c = self.full(1) if cid is None else self.C[cid]
            for i, v in enumerate(vec):
                if v * sign > 0:
                    row[i] = self.add(row[i], c)
                elif v * sign < 0:
                    row[i] = self.sub(row[i], c)
        return row

    def half_eval(self, half, v):
        """v: the half's four variables as exact int64 values [4, ...].  Returns (outputs as the kernel forms them: sums of
        centred products and plain sums; the centred products; the product operands)"""
        vals, opers = {}, {}
        for name, (cid, vec) in half.prod.items():
            y = sum(int(c) * v[i] for i, c in enumerate(vec) if c)
            opers[name] = y
            vals[name] = self.centre(self.mul(self.res(y), self.C[cid]))
        for name, vec in half.plain.items():
            vals[name] = sum(int(c) * v[i] for i, c in enumerate(vec) if c)
        outs = {o: sum(s * vals[name] for s, name in terms) for o, terms in half.out.items()}
        return outs, {k: vals[k] for k in half.prod}, opers

    def _half_inverse(self, half):
        """[4, 4, k, n]: the matrix taking the half's four outputs (ascending) back to its four variables"""
        key = id(half)
        if key not in self._inv_cache:
            A = np.stack([self.coef(half, half.out[o]) for o in sorted(half.out)])
            eye = np.stack([np.stack([self.full(int(i == j)) for j in range(4)]) for i in range(4)])
            self._inv_cache[key] = self.solve(A, eye)
        return self._inv_cache[key]

    def _apply(self, Minv, Y):
        """Minv [4, 4, k, n] times Y [4, ..., k, n]"""
        out = []
        for i in range(4):
            acc = self.mul(Minv[i, 0], Y[0])
            for j in range(1, 4):
                acc = self.add(acc, self.mul(Minv[i, j], Y[j]))
            out.append(acc)
        return out

    def _solve_half(self, half, rows, targets):
        """the half's variables [4, k, n] with functional rows[i] (a list of signed terms) = targets[i] per slot"""
        A = np.stack([self.coef(half, terms) for terms in rows])
        X, ok = self.solve(A, np.stack([t[None] for t in targets]))
        return X[:, 0], ok

    # -- the forward circuit as k_dct_rows / k_dct_cols evaluate it ---------------------------------------------------
    def fwd_line(self, V):
        """V int64 [8, ...]: the line's inputs.  Returns (outputs [8, ...], products, operands)"""
        a = np.stack([V[m] + V[7 - m] for m in range(4)])
        b = np.stack([V[3] - V[4], V[2] - V[5], V[1] - V[6], V[0] - V[7]])
        oe, pe, ye = self.half_eval(FWD_EVEN, a)
        oo, po, yo = self.half_eval(FWD_ODD, b)
        outs = {**oe, **oo}
        return np.stack([outs[i] for i in range(8)]), dict(pe, **po), dict(ye, **yo)

    def forward(self, X):
        """X: residues [8 rows, 8 cols, ..., k, n].  stored: the row outputs [row, col] as the packed variant stores them
        (0/4 reduced); operand: what the scale product of output [row, col] is given; final: the residues handed to the inverse
        transform."""
        rows, rprod, _ = self.fwd_line(np.moveaxis(self.centre(X), 1, 0))      # [col, row, ...]
        for o in (0, 4):
            rows[o] = self.centre(self.res(rows[o]))
        stored = np.moveaxis(rows, 0, 1)                                        # [row, col, ...]
        operand, cprod, _ = self.fwd_line(stored)                               # the column line runs along the rows
        final = self.mul(self.res(operand), self.fwd_scale.reshape((8, 8) + (1,) * (X.ndim - 4) + (self.k, self.n)))
        return dict(stored=stored, operand=operand, final=final, row_products=rprod, col_products=cprod)

    def fwd_line_invert(self, Y):
        """residues of a forward line's eight outputs [8, ..., k, n] -> residues of its inputs, and the solvable mask"""
        (Me, oke), (Mo, oko) = self._half_inverse(FWD_EVEN), self._half_inverse(FWD_ODD)
        a, b = self._apply(Me, Y[0::2]), self._apply(Mo, Y[1::2])               # b = (tmp4 .. tmp7), tmp_(7-m) = b[3 - m]
        d = [None] * 8
        for m in range(4):
            d[m] = self.mul(self.add(a[m], b[3 - m]), self.inv2)
            d[7 - m] = self.mul(self.sub(a[m], b[3 - m]), self.inv2)
        return np.stack(d), oke & oko

    # -- the inverse circuit as k_idct_rows / k_idct_cols evaluate it -------------------------------------------------
    def inv_halves(self, d):
        """d int64 [8, ...]: a line's inputs -> (E [4, ...], O [4, ...] before any reduction, products, operands)"""
        oe, pe, ye = self.half_eval(INV_EVEN, d[0::2])
        oo, po, yo = self.half_eval(INV_ODD, d[1::2])
        return np.stack([oe[i] for i in range(4)]), np.stack([oo[i] for i in range(4)]), dict(pe, **po), dict(ye, **yo)

    def inverse(self, X):
        """X: residues [8 rows, 8 cols, ..., k, n]"""
        scale = self.inv_scale.reshape((8, 8) + (1,) * (X.ndim - 4) + (self.k, self.n))
        scaled = self.centre(self.mul(X, scale))                                # the input products, [row, col, ...]
        E_pre, O_pre, rprod, _ = self.inv_halves(np.moveaxis(scaled, 1, 0))      # [m, row, ...]
        E, O = self.centre(self.res(E_pre)), self.centre(self.res(O_pre))
        col_in = np.stack([E[c] + O[c] if c < 4 else E[7 - c] - O[7 - c] for c in range(8)], axis=1)     # [row, col, ...]
        Ec, Oc, cprod, coper = self.inv_halves(col_in)                            # the column line runs along the rows
        out = np.stack([Ec[j] + Oc[j] if j < 4 else Ec[7 - j] - Oc[7 - j] for j in range(8)])
        return dict(scaled=scaled, E_pre=np.moveaxis(E_pre, 0, 1), O_pre=np.moveaxis(O_pre, 0, 1), E=np.moveaxis(E, 0, 1),
                    O=np.moveaxis(O, 0, 1), row_products=rprod, col_in=col_in, col_products=cprod, col_operands=coper,
                    out_pre=out, final=self.res(out))

    def inv_line_invert(self, Y):
        """residues of an inverse line's eight outputs [8, ..., k, n] -> residues of its (scaled) inputs, and the solvable mask"""
        (Me, oke), (Mo, oko) = self._half_inverse(INV_EVEN), self._half_inverse(INV_ODD)
        Eh = [self.mul(self.add(Y[m], Y[7 - m]), self.inv2) for m in range(4)]
        Oh = [self.mul(self.sub(Y[m], Y[7 - m]), self.inv2) for m in range(4)]
        a, b = self._apply(Me, Eh), self._apply(Mo, Oh)
        d = [None] * 8
        d[0::2], d[1::2] = a, b
        return np.stack(d), oke & oko

    # -- crafted blocks: each returns (residues of polynomial 0 [8 rows, 8 cols, k, n], solvable mask [k, n]) ---------
    def _fwd_extreme_lines(self):
        """F1 / F3 forward: line r aims at odd output {1,3,5,7}[r % 4] -- its four products = s h -- and, in the even half, at
        both products of output 2 (r even) or 6 (r odd) = s h, output 0 = s h, output 4 = -s h; s = +1 for r < 4, else -1;
        h = (p - 1) / 2.  Returns lines [8 (r), 8 inputs, k, n]."""
        h, ok = self.full([int(x) for x in self.H[:, 0]]), np.ones((self.k, self.n), dtype=bool)
        odd, even = {}, {}
        for o in FWD_ODD_OUTPUTS:
            odd[o], good = self._solve_half(FWD_ODD, [[t] for t in FWD_ODD.out[o]], [h] * 4)
            ok &= good
        for o in (2, 6):
            even[o], good = self._solve_half(FWD_EVEN, [[t] for t in FWD_EVEN.out[o]] + [FWD_EVEN.out[0], FWD_EVEN.out[4]], [h, h, h, self.neg(h)])
            ok &= good
        lines = []
        for r in range(8):
            a, b = even[6 if r % 2 else 2], odd[FWD_ODD_OUTPUTS[r % 4]]
            d = [None] * 8
            for m in range(4):
                d[m] = self.mul(self.add(a[m], b[3 - m]), self.inv2)
                d[7 - m] = self.mul(self.sub(a[m], b[3 - m]), self.inv2)
            d = np.stack(d)
            lines.append(self.neg(d) if r >= 4 else d)
        return np.stack(lines), ok

    def craft_fwd_f1(self):
        return self._fwd_extreme_lines()

    def craft_fwd_f3(self):
        """the extreme lines as the COLUMN lines' inputs (column c plays r), reached by inverting the row line"""
        lines, ok = self._fwd_extreme_lines()                       # [col, position along the column = row, k, n]
        X, good = self.fwd_line_invert(lines)                       # row outputs indexed [col, row] -> row inputs [col', row]
        return np.moveaxis(X, 0, 1), ok & good

    def craft_fwd_f4(self, G):
        """G [8, 8, k, n]: the residues wanted at the input of the inverse transform"""
        sinv, nz = self._scale_inverse("fwd_scale")
        cols, ok1 = self.fwd_line_invert(self.mul(G, sinv))         # along the rows: column lines
        X, ok2 = self.fwd_line_invert(np.moveaxis(cols, 1, 0))      # [col, row] -> inputs [col', row]
        return np.moveaxis(X, 0, 1), nz.all((0, 1)) & ok1 & ok2

    def _scale_inverse(self, which):
        if which not in self._inv_cache:
            self._inv_cache[which] = self.inv(getattr(self, which))
        return self._inv_cache[which]

    def _unscale(self, d):
        sinv, nz = self._scale_inverse("inv_scale")
        return self.mul(d, sinv), nz.all((0, 1))

    def craft_inv_f1(self):
        """row r: the four products of O[r % 4] = s h; even half: the scaled d0 = s h and both products of t3 = s h with d4 = s h
        (r even: t0 and t3 reach s (p - 1), E0 reaches s (2 p - 2)) or both products of t2 = s h with d4 = -s h (r odd: t1, t2, E1).
        d2 and d6 are two unknowns, so only two of the three even products can be pinned: hence the alternation."""
        h, ok = self.full([int(x) for x in self.H[:, 0]]), np.ones((self.k, self.n), dtype=bool)
        odd, even = [], []
        for m in range(4):
            b, good = self._solve_half(INV_ODD, [[t] for t in INV_ODD.out[m]], [h] * 4)
            odd.append(b)
            ok &= good
        for second, d4 in (("e2", h), ("e1", self.neg(h))):
            a, good = self._solve_half(INV_EVEN, [[(1, "d0")], [(1, "d4")], [(1, "e0")], [(1, second)]], [h, d4, h, h])
            even.append(a)
            ok &= good
        rows = []
        for r in range(8):
            d = [None] * 8
            d[0::2], d[1::2] = list(even[r % 2]), list(odd[r % 4])
            d = np.stack(d)
            rows.append(self.neg(d) if r >= 4 else d)
        X, good = self._unscale(np.stack(rows))
        return X, ok & good

    def craft_inv_f3(self, o_sign):
        """every stored E[m] = h and O[m] = o_sign h in every row: the column inputs E + O (columns 0..3) or E - O (4..7) are
        p - 1, the others 0, and z3 + z4 of those columns is 4 (p - 1)"""
        h = self.full([int(x) for x in self.H[:, 0]])
        (Me, oke), (Mo, oko) = self._half_inverse(INV_EVEN), self._half_inverse(INV_ODD)
        a, b = self._apply(Me, [h] * 4), self._apply(Mo, [h if o_sign > 0 else self.neg(h)] * 4)
        d = [None] * 8
        d[0::2], d[1::2] = a, b
        X, good = self._unscale(np.broadcast_to(np.stack(d), (8, 8, self.k, self.n)))
        return X, oke & oko & good

    def craft_inv_f4(self, G):
        cols, ok1 = self.inv_line_invert(G)                          # along the rows: column lines; = the row lines' outputs
        d, ok2 = self.inv_line_invert(np.moveaxis(cols, 1, 0))       # [col, row] -> scaled inputs [col', row]
        X, good = self._unscale(np.moveaxis(d, 0, 1))
        return X, ok1 & ok2 & good

    def solver_left_out(self):
        """slots (of k n) at which any system that the families solve is singular: the extreme lines of both directions, the four
        half-line inverses and the inverses of both scale tables"""
        ok = self._fwd_extreme_lines()[1] & self.craft_inv_f1()[1] & self._scale_inverse("fwd_scale")[1].all((0, 1))
        for half in (FWD_EVEN, FWD_ODD, INV_EVEN, INV_ODD):
            ok = ok & self._half_inverse(half)[1]
        return int((~ok).sum())

    # -- slot patterns of F4 ----------------------------------------------------------------------------------------
    def f4_bits(self, every_bit):
        logn = self.n.bit_length() - 1
        return list(range(logn)) if every_bit else [0, logn - 1]

    def f4_pattern(self, bit):
        """[k, n]: +(p - 1) / 2 at every slot (bit None), or -(p - 1) / 2 where `bit` of the oracle's slot index is set"""
        h = self.full([int(x) for x in self.H[:, 0]])
        if bit is None:
            return h
        return np.where(((np.arange(self.n) >> bit) & 1).astype(bool)[None, :], self.neg(h), h)

    def f4_targets(self, every_bit):
        """[8, 8, k, n]: output 8 row + col carries pattern (8 row + col) mod (1 + number of bits); the pattern list"""
        pats = [None] + self.f4_bits(every_bit)
        G = np.stack([self.f4_pattern(pats[i % len(pats)]) for i in range(64)]).reshape(8, 8, self.k, self.n)
        return G, pats

    # -- back to coefficients -----------------------------------------------------------------------------------------
    def to_slots(self, block):
        """[64, 2, k, n] coefficients -> [8, 8, 2, k, n] residues at the slots"""
        out = np.empty_like(block)
        for idx in np.ndindex(block.shape[:2]):
            for i in range(self.k):
                out[idx][i] = self.orc.ntt_fwd(block[idx][i], i)
        return out.reshape(8, 8, 2, self.k, self.n)

    def block(self, crafted, rng):
        """(slots of polynomial 0 [8, 8, k, n], solvable mask) -> ciphertext block [64, 2, k, n] in coefficient form; polynomial 1
        carries the negated pattern.  Slots the solver left out keep random values and are counted against MAX_LEFT_OUT."""
        X, ok = crafted
        bad = int((~ok).sum())
        self.left_out += bad
        self.crafted += ok.size
        assert bad <= MAX_LEFT_OUT * ok.size, "the solver left out %d of %d slots" % (bad, ok.size)
        if bad:
            rnd = (rng.integers(0, 1 << 62, size=X.shape, dtype=np.int64).astype(U)) % self.P
            X = np.where(ok, X, rnd)
        S = np.stack([X, self.neg(X)], axis=2).reshape(64, 2, self.k, self.n)
        out = np.empty_like(S)
        for idx in np.ndindex(64, 2):
            for i in range(self.k):
                out[idx][i] = self.orc.ntt_inv(S[idx][i], i)
        return out

    def constant_block(self, values):
        """F2: ciphertext i is the constant polynomial values[i] (a list of per-prime residues) x^0, polynomial 1 its negation"""
        out = np.zeros((64, 2, self.k, self.n), dtype=U)
        for i, v in enumerate(values):
            for j, p in enumerate(self.q):
                out[i, 0, j, 0] = v[j] % p
                out[i, 1, j, 0] = (-v[j]) % p
        return out

    def f2_constants(self):
        """name -> 64 lists of per-prime residues: 1, (p - 1) / 2, (p + 1) / 2, p - 1 everywhere, and the two ties alternating"""
        lo, hi = [(p - 1) // 2 for p in self.q], [(p + 1) // 2 for p in self.q]
        return {"one": [[1] * self.k] * 64, "half-": [lo] * 64, "half+": [hi] * 64, "top": [[p - 1 for p in self.q]] * 64,
                "ties": [lo if i % 2 == 0 else hi for i in range(64)]}


def craft_batch(model, direction, every_bit, seed=2026):
    """One direction's crafted batch for the model's (n, primes): (family name of each block, blocks [9, 64, 2, k, n], F4 targets
    G [8, 8, k, n], F4 pattern list).  Nine blocks: an odd count gives a ragged last wave at two blocks per wave."""
    m, rng = model, np.random.default_rng(seed)
    G, pats = m.f4_targets(every_bit)
    f2 = [("F2-" + k, m.constant_block(v)) for k, v in m.f2_constants().items()]
    if direction == "fwd":
        blocks = [("F1", m.block(m.craft_fwd_f1(), rng))] + f2 + [("F3", m.block(m.craft_fwd_f3(), rng)), ("F4", m.block(m.craft_fwd_f4(G), rng)),
                                                                  ("random", m.orc.random_ct(64, seed=seed))]
    else:
        blocks = [("F1", m.block(m.craft_inv_f1(), rng))] + f2 + [("F3", m.block(m.craft_inv_f3(+1), rng)), ("F3-diff", m.block(m.craft_inv_f3(-1), rng)),
                                                                  ("F4", m.block(m.craft_inv_f4(G), rng))]
    return [a for a, _ in blocks], np.stack([b for _, b in blocks]), G, pats
