"""Specification of the baby-step / giant-step linear maps on encrypted slots (include/fhe_hip.h: fhe_rotate_bsgs_sp), restated on the
UNCHANGED CPU oracle: only Oracle.ntt_fwd / ntt_inv per prime, Oracle.plain_lift, Python-integer slot products, tests/modswitch_oracle.py's
drop, tests/galois_oracle.py's sigma and tests/rotsum_oracle.py's slot permutation.  Nothing here calls the library.

The setting is tests/rotdiag_oracle.py's.  Baby elements g_j with keys KB_j, giant elements h_i with keys KG_i, plaintexts p_(i,j)
[G2][G1][n] modulo t (all zero = the pair is absent), P_(i,j),r = NTT_(q_r)(centred lift):
  A(i)_pp,r = sum_(j present) P_(i,j),r (*) [ sum_l pi_(g_j)(D_l,r) (*) KB_j,l,pp,r + [pp=0, r<L] [p] pi_(g_j)(C0_r) + [pp=1, g_j=1, r<L] [p] D_r,r ]
  v(i)      = one drop of A(i)_1 (h_i != 1),   E(i)_l,r = NTT_(q_r)([v(i)_l]_(q_r))
  B_pp,r    = sum_(i: h_i != 1) [ sum_l pi_(h_i)(E(i)_l,r) (*) KG_i,l,pp,r + [pp=0] pi_(h_i)(A(i)_0,r) ] + sum_(i: h_i = 1) A(i)_pp,r
  out_pp    = one drop of B_pp
Two forms: residues on the oracle's transforms (the GPU tests' reference) and big integers modulo Q p (small n), with the WRONG variants."""
import numpy as np

import galois_oracle as go
import keyswitch_sp_oracle as ks
import modswitch_oracle as mo
import rotdiag_oracle as rd
import rotsum_oracle as rs

VARIANTS = ("galois_digit", "a0_dropped", "a0_no_perm", "perm_inv", "giant_first", "id_switched")
MAX_STEPS = 64
_obj, _u64 = rs._obj, rs._u64


def _check_elts(n, elts, what):
    if not 1 <= len(elts) <= MAX_STEPS:
        return "%s step count" % what
    for j, g in enumerate(elts):
        if not (g & 1) or not 0 < g < 2 * n:
            return "%s Galois element %d: must be odd" % (what, g)
        if g in elts[:j]:
            return "%s Galois element %d is repeated" % (what, g)
    return None


def present(plains):
    """[G2][G1] bool"""
    return [[bool(any(int(v) for v in p)) for p in row] for row in plains]


def check_plan(n, t, k, baby, giant, plains):
    """the refusals of fhe_rotbsgs_plan_create that need no device: the reason, or None"""
    if k < 2:
        return "at least 2 primes"
    why = _check_elts(n, list(baby), "baby") or _check_elts(n, list(giant), "giant")
    if why:
        return why
    if len(plains) != len(giant) or any(len(row) != len(baby) for row in plains):
        return "plaintexts [G2][G1][n] expected"
    for i, row in enumerate(plains):
        for j, p in enumerate(row):
            if len(p) != n:
                return "plaintext of pair (%d, %d): %d coefficients" % (i, j, len(p))
            if any(int(v) >= t or int(v) < 0 for v in p):
                return "plaintext of pair (%d, %d): coefficient is not below t" % (i, j)
    pr = present(plains)
    for i in range(len(giant)):
        if not any(pr[i]):
            return "giant step %d has no present pair" % i
    for j in range(len(baby)):
        if not any(pr[i][j] for i in range(len(giant))):
            return "baby step %d has no present pair" % j
    return None


def _perm(orc, g, r, variant):
    return rs.slot_perm(orc, pow(g, -1, 2 * orc.n) if variant == "perm_inv" else g, r)


def _drop1(orc, acc_ntt):
    """acc_ntt [k] object arrays in NTT form -> [L][n] uint64: the inverse transforms and one drop"""
    x = np.stack([orc.ntt_inv(_u64(acc_ntt[r]), r) for r in range(orc.k)])
    return mo.switch_residues_levels(x, orc.q)[orc.k - 1]


def inner_sums(orc, ct, t, baby, plains, kb, variant=None, giant=None):
    """A [G2][2][k] object arrays in NTT form"""
    k, n, q = orc.k, orc.n, orc.q
    L, p = k - 1, q[-1]
    D = rs.digits(orc, ct[1])
    C0 = [_obj(orc.ntt_fwd(ct[0, r], r)) for r in range(L)]
    pr = present(plains)
    Tc = {}

    def T_of(j, pp, r):
        """T_j,pp,r: what every giant step shares of baby step j"""
        if (j, pp, r) not in Tc:
            g = baby[j]
            perm = _perm(orc, g, r, variant)
            T = np.zeros(n, dtype=object)
            if g != 1:
                T = sum(D[r][l][perm] * _obj(kb[j][l, pp, r]) for l in range(L)) % q[r]
            if r < L and pp == 0:
                T = (T + (p % q[r]) * C0[r][perm]) % q[r]
            if r < L and pp == 1 and g == 1:
                T = (T + (p % q[r]) * D[r][r]) % q[r]
            Tc[(j, pp, r)] = T
        return Tc[(j, pp, r)]

    A = []
    for i, row in enumerate(plains):
        idx = [j for j in range(len(baby)) if pr[i][j]]
        P = dict(zip(idx, rd.transforms(orc, rd.lifts(orc, [row[j] for j in idx], t))))
        Ai = [[np.zeros(n, dtype=object) for _ in range(k)] for _ in range(2)]
        for r in range(k):
            for j in idx:
                Pr = P[j][r]
                if variant == "giant_first" and giant[i] != 1:          # rot_h(rot_g(ct)) times the diagonal: the diagonal is not rotated
                    Pr = Pr[rs.slot_perm(orc, pow(giant[i], -1, 2 * n), r)]
                for pp in range(2):
                    Ai[pp][r] = (Ai[pp][r] + Pr * T_of(j, pp, r)) % q[r]
        A.append(Ai)
    return A


def rotate_bsgs(orc, ct, t, baby, giant, plains, kb, kg, variant=None):
    """ct [2][L][n]; baby [G1], giant [G2]; plains [G2][G1][n] modulo t; kb [G1], kg [G2]: [L][2][k][n] in the oracle's NTT form (anything
    for the element 1; variant "id_switched" reads kg of the identity giant) -> [2][L][n]"""
    ct = np.asarray(ct, dtype=np.uint64)
    k, n, q = orc.k, orc.n, orc.q
    L, p = k - 1, q[-1]
    assert ct.shape == (2, L, n) and check_plan(n, t, k, list(baby), list(giant), plains) is None
    A = inner_sums(orc, ct, t, baby, plains, kb, variant, giant)
    B = [[np.zeros(n, dtype=object) for _ in range(k)] for _ in range(2)]
    for i, h in enumerate(giant):
        if h == 1 and variant != "id_switched":
            for pp in range(2):
                for r in range(k):
                    B[pp][r] = (B[pp][r] + A[i][pp][r]) % q[r]
            continue
        v = _drop1(orc, A[i][1])                                         # [L][n] canonical coefficients
        a0d = _drop1(orc, A[i][0]) if variant == "a0_dropped" else None
        for r in range(k):
            perm = np.arange(n) if h == 1 else _perm(orc, h, r, variant)
            for l in range(L):
                if variant == "galois_digit" and h != 1:                # fhe_apply_galois_sp's digit: sigma with the negation modulo q_l, then the reduction
                    E = _obj(orc.ntt_fwd(go.sigma(v[l][None], h, [q[l]])[0] % np.uint64(q[r]), r))
                else:
                    E = _obj(orc.ntt_fwd(v[l] % np.uint64(q[r]), r))[perm]
                for pp in range(2):
                    B[pp][r] = (B[pp][r] + E * _obj(kg[i][l, pp, r])) % q[r]
            if variant == "a0_dropped":
                if r < L:
                    B[0][r] = (B[0][r] + (p % q[r]) * _obj(orc.ntt_fwd(a0d[r], r))[perm]) % q[r]
            elif variant == "a0_no_perm":
                B[0][r] = (B[0][r] + A[i][0][r]) % q[r]
            else:
                B[0][r] = (B[0][r] + A[i][0][r][perm]) % q[r]
    return np.stack([_drop1(orc, B[pp]) for pp in range(2)])


# ---- big integers through CRT --------------------------------------------------------------------------------------------------------------
def rotate_bsgs_composed(q, t, c, baby, giant, plains, KB, KG):
    """c [2][n] integers modulo Q; plains [G2][G1][n] modulo t; KB [G1], KG [G2]: [L][2][n] integers modulo Q p (None for the element 1)
    -> [2][n] modulo Q.  Everything modulo Q p: the inner sums with the input's terms times p, ONE rounding division of A(i)_1 per
    non-identity giant step, the giant key switch on the digits sigma_h([v]_(q_l)) over Z, sigma_h of A(i)_0 as it is, ONE final rounding"""
    L, n = len(q) - 1, len(c[0])
    Qp, Q, p = mo.prod(q), mo.prod(q[:-1]), q[-1]
    pr = present(plains)
    T = []                                                               # per baby step: [2][n] modulo Q p
    for g, Kj in zip(baby, KB):
        s0 = c[0] if g == 1 else ks.sigma_big(c[0], g, Q)
        Tj = [[p * x % Qp for x in s0], [p * x % Qp for x in c[1]] if g == 1 else [0] * n]
        if g != 1:
            for l in range(L):
                d = [v % Qp for v in rs.sigma_signed([x % q[l] for x in c[1]], g)]
                for pp in range(2):
                    Tj[pp] = [(x + y) % Qp for x, y in zip(Tj[pp], mo.negacyclic_mul(d, Kj[l][pp], Qp))]
        T.append(Tj)
    B = [[0] * n, [0] * n]
    for i, h in enumerate(giant):
        A = [[0] * n, [0] * n]
        for j in range(len(baby)):
            if not pr[i][j]:
                continue
            pc = [v % Qp for v in rd.centred_poly(plains[i][j], t)]
            for pp in range(2):
                A[pp] = [(x + y) % Qp for x, y in zip(A[pp], mo.negacyclic_mul(pc, T[j][pp], Qp))]
        if h == 1:
            B = [[(x + y) % Qp for x, y in zip(B[pp], A[pp])] for pp in range(2)]
            continue
        v = [mo.drop_big(x, q) for x in A[1]]
        B[0] = [(x + y) % Qp for x, y in zip(B[0], ks.sigma_big(A[0], h, Qp))]
        for l in range(L):
            d = [x % Qp for x in rs.sigma_signed([x % q[l] for x in v], h)]
            for pp in range(2):
                B[pp] = [(x + y) % Qp for x, y in zip(B[pp], mo.negacyclic_mul(d, KG[i][l][pp], Qp))]
    return [[mo.drop_big(x, q) for x in B[pp]] for pp in range(2)]


def _compose_keys(q, elts, keys_coeff, n):
    k, L = len(q), len(q) - 1
    return [None if g == 1 else [[[mo.compose([int(kc[l, pp, r, x]) for r in range(k)], q) for x in range(n)] for pp in range(2)] for l in range(L)]
            for g, kc in zip(elts, keys_coeff)]


def rotate_bsgs_big(q, t, ct, baby, giant, plains, kb_coeff, kg_coeff):
    """the same from residues (small n) -> residues [2][L][n]"""
    L = len(q) - 1
    n = np.asarray(ct).shape[-1]
    c = [[mo.compose([int(ct[pp][r][x]) for r in range(L)], q[:-1]) for x in range(n)] for pp in range(2)]
    out = rotate_bsgs_composed(q, t, c, baby, giant, plains, _compose_keys(q, baby, kb_coeff, n), _compose_keys(q, giant, kg_coeff, n))
    return np.array([[[v % qi for v in out[pp]] for qi in q[:-1]] for pp in range(2)], dtype=np.uint64)


# ---- plaintext families ----------------------------------------------------------------------------------------------------------------------
def plain_families(n, t, G1, G2, seed, absent=()):
    """name -> [G2][G1][n] plaintexts (rotdiag_oracle.plain_families per giant step); the pairs in `absent` are all zero"""
    out = {}
    fams = [rd.plain_families(n, t, G1, seed + 31 * i) for i in range(G2)]
    for name in ("dense", "top", "mask"):
        a = np.stack([np.stack(f[name]) for f in fams]).astype(np.uint64)
        for i, j in absent:
            a[i, j] = 0
        out[name] = a
    return out
