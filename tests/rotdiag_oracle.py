"""Specification of the diagonal linear maps on encrypted slots (include/fhe_hip.h: fhe_rotate_diag_sum_sp), restated on the UNCHANGED CPU
oracle: only Oracle.ntt_fwd / ntt_inv per prime, Oracle.plain_lift, Python-integer slot products, tests/modswitch_oracle.py's drop,
tests/galois_oracle.py's sigma and tests/rotsum_oracle.py's slot permutation.  Nothing here calls the library.

The setting is tests/rotsum_oracle.py's.  Taps (g_j, p_j, K_j): p_j a plaintext of n coefficients modulo t, p'_j its centred lift,
P_j,r = NTT_(q_r)(p'_j):
  acc_pp,r = sum_(j: g_j != 1) P_j,r (*) sum_i pi_(g_j)(D_i,r) (*) K_j,i,pp,r mod q_r,   u_pp = one drop (k -> k - 1) of acc_pp
  out      = (u_0 + sum_j p'_j sigma_(g_j)(c_0),  u_1 + sum_(j: g_j = 1) p'_j c_1)
Three forms: residues on the oracle's transforms (the GPU tests' reference), big integers modulo Q p (small n), and the structure the
kernels use (the input's terms inside the accumulator, times the special prime, before ONE drop), with the WRONG variants."""
import numpy as np

import galois_oracle as go
import keyswitch_sp_oracle as ks
import modswitch_oracle as mo
import rotsum_oracle as rs

VARIANTS = ("diag_first", "perm_inv", "uncentred", "c0_special", "no_id_c1")
_obj, _u64 = rs._obj, rs._u64


def check_taps(n, t, k, elts, plains):
    """the refusals of fhe_rotdiag_plan_create that need no device: the reason, or None"""
    why = rs.check_taps(n, t, k, list(elts), [1] * len(elts))
    if why:
        return why
    if len(plains) != len(elts):
        return "one plaintext per tap"
    for j, p in enumerate(plains):
        if len(p) != n:
            return "plaintext of tap %d: %d coefficients" % (j, len(p))
        if any(int(v) >= t or int(v) < 0 for v in p):
            return "plaintext of tap %d: coefficient is not below t" % j
        if not any(int(v) for v in p):
            return "plaintext of tap %d is the zero polynomial" % j
    return None


def constant(n, w):
    """the constant polynomial w"""
    p = np.zeros(n, dtype=np.uint64)
    p[0] = w
    return p


def centred_poly(p, t):
    return [rs.centred(v, t) for v in p]


def lifts(orc, plains, t, uncentred=False):
    """[G][k][n] uint64: the lift of every plaintext to every prime -- Oracle.plain_lift (the centred lift of fhe_multiply_plain), or the
    WRONG uncentred one"""
    assert orc.t == t
    if uncentred:
        return [np.stack([np.asarray(p, dtype=np.uint64) % np.uint64(qr) for qr in orc.q]) for p in plains]
    out = [orc.plain_lift(np.asarray(p, dtype=np.uint64)) for p in plains]
    for p, lp in zip(plains, out):                                       # plain_lift IS the centred lift (t odd)
        assert [int(v) for v in lp[0][:4]] == [rs.centred(v, t) % orc.q[0] for v in p[:4]]
    return out


def transforms(orc, lifted):
    """[G][k] object arrays: P_j,r in the oracle's slot order"""
    return [[_obj(orc.ntt_fwd(lp[r], r)) for r in range(orc.k)] for lp in lifted]


def accumulators(orc, D, elts, P, keys, variant=None):
    """acc [2][k][n] in NTT form, object arrays modulo q_r"""
    k, n, q = orc.k, orc.n, orc.q
    acc = [[np.zeros(n, dtype=object) for _ in range(k)] for _ in range(2)]
    for r in range(k):
        for pp in range(2):
            s = np.zeros(n, dtype=object)
            for g, Pj, key in zip(elts, P, keys):
                if g == 1:
                    continue
                perm = rs.slot_perm(orc, pow(g, -1, 2 * n) if variant == "perm_inv" else g, r)
                if variant == "diag_first":                              # rotate(multiply_plain(ct, p)): the diagonal is permuted too
                    s = (s + Pj[r][perm] * sum(D[r][i][perm] * _obj(key[i, pp, r]) for i in range(k - 1))) % q[r]
                else:
                    s = (s + Pj[r] * sum(D[r][i][perm] * _obj(key[i, pp, r]) for i in range(k - 1))) % q[r]
            acc[pp][r] = s
    return acc


def _coeff(orc, acc):
    return np.stack([np.stack([orc.ntt_inv(_u64(acc[pp][r]), r) for r in range(orc.k)]) for pp in range(2)])


def input_terms(orc, ct, elts, P, variant=None):
    """(Z_0 [L], Z_1 [L]) in NTT form: Z_0,r = sum_j P_j,r (*) NTT(sigma_(g_j)(c_0,r)), Z_1,r = P_id,r (*) NTT(c_1,r)"""
    L, n, q = orc.k - 1, orc.n, orc.q
    Z0, Z1 = [], []
    for r in range(L):
        z0, z1 = np.zeros(n, dtype=object), np.zeros(n, dtype=object)
        for g, Pj in zip(elts, P):
            ge = pow(g, -1, 2 * n) if variant == "perm_inv" else g
            sg = rs._sigma1(ct[0, r][None], ge, [q[r]])[0]
            Pr = Pj[r][rs.slot_perm(orc, g, r)] if variant == "diag_first" and g != 1 else Pj[r]
            z0 = (z0 + Pr * _obj(orc.ntt_fwd(sg, r))) % q[r]
            if g == 1 and variant != "no_id_c1":
                z1 = (z1 + Pj[r] * _obj(orc.ntt_fwd(ct[1, r], r))) % q[r]
        Z0.append(z0)
        Z1.append(z1)
    return Z0, Z1


def rotate_diag_sum(orc, ct, t, elts, plains, keys, variant=None):
    """ct [2][L][n]; elts [G]; plains [G][n] modulo t; keys [G]: [L][2][k][n] in the oracle's NTT form (anything for g = 1) -> [2][L][n].
    The specification as stated: the drop of the accumulators, then the input's terms added modulo q_r."""
    ct = np.asarray(ct, dtype=np.uint64)
    k, n, q = orc.k, orc.n, orc.q
    L = k - 1
    assert ct.shape == (2, L, n) and check_taps(n, t, k, list(elts), plains) is None
    if variant == "c0_special":
        return rotate_diag_sum_structured(orc, ct, t, elts, plains, keys, c0_special=True)
    P = transforms(orc, lifts(orc, plains, t, uncentred=variant == "uncentred"))
    u = rs._drop(_coeff(orc, accumulators(orc, rs.digits(orc, ct[1]), elts, P, keys, variant)), q)
    Z0, Z1 = input_terms(orc, ct, elts, P, variant)
    out = np.zeros_like(ct)
    for r in range(L):
        out[0, r] = _u64((_obj(u[0, r]) + _obj(orc.ntt_inv(_u64(Z0[r]), r))) % q[r])
        out[1, r] = _u64((_obj(u[1, r]) + _obj(orc.ntt_inv(_u64(Z1[r]), r))) % q[r])
    return out


def rotate_diag_sum_structured(orc, ct, t, elts, plains, keys, c0_special=False):
    """the suggested structure: acc'_pp,r = acc_pp,r + [p]_(q_r) Z_pp,r for r < L, the special prime's row as it is, ONE drop, nothing
    added afterwards.  c0_special (WRONG): the c_0 term also enters the special prime's row, as if it were one more low prime reading
    residue 0 of c_0"""
    ct = np.asarray(ct, dtype=np.uint64)
    k, n, q = orc.k, orc.n, orc.q
    L, p = k - 1, q[-1]
    P = transforms(orc, lifts(orc, plains, t))
    acc = accumulators(orc, rs.digits(orc, ct[1]), elts, P, keys)
    Z0, Z1 = input_terms(orc, ct, elts, P)
    for r in range(L):
        acc[0][r] = (acc[0][r] + (p % q[r]) * Z0[r]) % q[r]
        acc[1][r] = (acc[1][r] + (p % q[r]) * Z1[r]) % q[r]
    if c0_special:
        z = np.zeros(n, dtype=object)
        for g, Pj in zip(elts, P):
            z = (z + Pj[L] * _obj(orc.ntt_fwd(rs._sigma1((ct[0, 0] % np.uint64(p))[None], g, [p])[0], L))) % p
        acc[0][L] = (acc[0][L] + (q[0] % p) * z) % p
    return rs._drop(_coeff(orc, acc), q)


# ---- big integers through CRT --------------------------------------------------------------------------------------------------------------
def rotate_diag_sum_composed(q, t, c, elts, plains, K):
    """c [2][n] integers modulo Q; plains [G][n] modulo t; K [G]: [L][2][n] integers modulo Q p (None for g = 1) -> [2][n] modulo Q: the
    digits sigma_g(d_i) over Z, the products with the centred plaintexts modulo Q p, ONE rounding division by p, then the additions"""
    L, n = len(q) - 1, len(c[0])
    Qp, Q = mo.prod(q), mo.prod(q[:-1])
    pc = [centred_poly(p, t) for p in plains]
    acc = [[0] * n, [0] * n]
    for g, pj, Kj in zip(elts, pc, K):
        if g == 1:
            continue
        inner = [[0] * n, [0] * n]
        for i in range(L):
            d = [v % Qp for v in rs.sigma_signed([x % q[i] for x in c[1]], g)]
            for pp in range(2):
                inner[pp] = [(x + y) % Qp for x, y in zip(inner[pp], mo.negacyclic_mul(d, Kj[i][pp], Qp))]
        for pp in range(2):
            acc[pp] = [(x + y) % Qp for x, y in zip(acc[pp], mo.negacyclic_mul([v % Qp for v in pj], inner[pp], Qp))]
    out = [[mo.drop_big(v, q) for v in acc[pp]] for pp in range(2)]
    for g, pj in zip(elts, pc):
        pq = [v % Q for v in pj]
        s0 = c[0] if g == 1 else ks.sigma_big(c[0], g, Q)
        out[0] = [(x + y) % Q for x, y in zip(out[0], mo.negacyclic_mul(pq, s0, Q))]
        if g == 1:
            out[1] = [(x + y) % Q for x, y in zip(out[1], mo.negacyclic_mul(pq, c[1], Q))]
    return out


def rotate_diag_sum_big(q, t, ct, elts, plains, keys_coeff):
    """the same from residues (small n) -> residues [2][L][n]"""
    k, L = len(q), len(q) - 1
    n = np.asarray(ct).shape[-1]
    K = [None if g == 1 else [[[mo.compose([int(kc[i, pp, r, x]) for r in range(k)], q) for x in range(n)] for pp in range(2)] for i in range(L)]
         for g, kc in zip(elts, keys_coeff)]
    c = [[mo.compose([int(ct[pp][r][x]) for r in range(L)], q[:-1]) for x in range(n)] for pp in range(2)]
    out = rotate_diag_sum_composed(q, t, c, elts, plains, K)
    return np.array([[[v % qi for v in out[pp]] for qi in q[:-1]] for pp in range(2)], dtype=np.uint64)


# ---- plaintext families ----------------------------------------------------------------------------------------------------------------------
def border_mask_slots(n, tile_w, j):
    """0/1 slot values, flat row order: 0 in column (j mod tile_w) of every tile row, 1 elsewhere (never all zero)"""
    s = np.ones(n, dtype=np.uint64)
    s[(j % tile_w)::tile_w] = 0
    return s


def plain_families(n, t, G, seed):
    """name -> [G][n] plaintexts: random dense; (t - 1) X^(n-1); the encodings of 0/1 border masks in the slots"""
    rng = np.random.default_rng(seed)
    dense = [rng.integers(0, t, size=n, dtype=np.uint64) for _ in range(G)]
    top = []
    for _ in range(G):
        p = np.zeros(n, dtype=np.uint64)
        p[n - 1] = t - 1
        top.append(p)
    mask = [np.asarray(go.encode_slots([int(v) for v in border_mask_slots(n, 32, j)], n, t), dtype=np.uint64) for j in range(G)]
    return {"dense": dense, "top": top, "mask": mask}
