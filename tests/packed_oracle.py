"""Specification of the integer linear maps across slot-packed ciphertexts (include/fhe_hip.h: fhe_block8x8_scalar, fhe_channel_mix), twice:
as the op-by-op composition on the UNCHANGED CPU oracle (multiply_plain with a one-coefficient plaintext, add, add_plain), and as a direct
integer evaluation modulo each q_i in numpy, for speed.  tests/test_packed_cpu.py checks that the two agree; the GPU tests compare the
library's bits with the direct form.  Nothing here calls the library."""
import numpy as np

T33 = 4295294977          # 0x100050001: prime, = 1 (mod 32768): the 33-bit batching modulus of the tests
T41 = 0x10000048001       # prime, = 1 (mod 32768): holds the colour mix in front of the forward plan (bound 4.2e11 < t / 2)
W_MAX = (1 << 31) - 1


def scalar_limit(t):
    return min((t - 1) // 2, W_MAX)


def random_plan(rng, t, pre=True, post=True):
    """L, R (with zeros inside and both ends of the range), pre, post (no zeros) over the whole allowed range"""
    lim = scalar_limit(t)
    L, R = (rng.integers(-lim, lim + 1, size=(8, 8), dtype=np.int64) for _ in range(2))
    L[0, 0], L[0, 1], L[3, 4], L[7, 7] = lim, -lim, 0, 0
    R[1, 1], R[2, 0], R[5, 5], R[6, :7] = -lim, lim, 0, 0          # row 6 of R keeps one entry
    R[6, 7] = R[6, 7] or 1
    out = [L, R]
    for want in (pre, post):
        if not want:
            out.append(None)
            continue
        p = rng.integers(-lim, lim + 1, size=(8, 8), dtype=np.int64)
        p[p == 0] = 1
        p[0, 0], p[7, 7], p[1, 2], p[2, 1] = lim, -lim, 1, -1
        out.append(p)
    return out


# ---- 1. the composition on the oracle ------------------------------------------------------------------------------------------------
def _scalar(orc, a, w):
    """multiply_plain with the one-coefficient plaintext [w mod t]"""
    return orc.multiply_plain(a, np.array([int(w) % orc.t], dtype=np.uint64))


def _weighted_sum(orc, terms):
    acc = None
    for w, a in terms:
        if int(w) == 0:
            continue                                                   # a zero entry is a skipped term
        term = _scalar(orc, a, w)
        acc = term if acc is None else orc.add(acc, term)
    assert acc is not None, "an all-zero row is refused by the library"
    return acc


def block8x8_compose(orc, X, L, R, pre=None, post=None):
    """X: [64][size, k, n] (ciphertext 8 x + y is X[x][y]).  pre per input, L down the columns, R along the rows, post per output."""
    x = [[X[8 * i + j] if pre is None else _scalar(orc, X[8 * i + j], pre[i][j]) for j in range(8)] for i in range(8)]
    cols = [[_weighted_sum(orc, [(L[u][i], x[i][y]) for i in range(8)]) for y in range(8)] for u in range(8)]
    out = []
    for u in range(8):
        for v in range(8):
            y = _weighted_sum(orc, [(R[v][j], cols[u][j]) for j in range(8)])
            out.append(y if post is None else _scalar(orc, y, post[u][v]))
    return np.stack(out)


def channel_mix_compose(orc, M, planes, bias=None):
    """planes: [c][size, k, n]; out_i = sum_j M[i][j] planes_j, then add_plain of [bias_i mod t] when bias_i != 0"""
    out = []
    for i, row in enumerate(M):
        y = _weighted_sum(orc, [(w, planes[j]) for j, w in enumerate(row)])
        if bias is not None and int(bias[i]) != 0:
            y = orc.add_plain(y, np.array([int(bias[i]) % orc.t], dtype=np.uint64))
        out.append(y)
    return np.stack(out)


# ---- 2. the direct evaluation modulo q_i -----------------------------------------------------------------------------------------------
def mulmod(a, w, q):
    """a * w mod q for a uint64 array below 2^63 (not necessarily reduced) and a Python integer 0 <= w < q < 2^61: the quotient from an
    80-bit float estimate (off by at most one), the remainder in wrapping 64-bit arithmetic"""
    a = np.asarray(a, dtype=np.uint64)
    qh = np.floor(a.astype(np.longdouble) * np.longdouble(w) / np.longdouble(q)).astype(np.uint64)
    with np.errstate(over="ignore"):
        r = (a * np.uint64(w) - qh * np.uint64(q)).view(np.int64)
    r = np.where(r < 0, r + np.int64(q), r)
    r = np.where(r >= np.int64(q), r - np.int64(q), r)
    assert ((r >= 0) & (r < q)).all()
    return r.astype(np.uint64)


def _lin(terms, q):
    """sum of w * a over (w, a) modulo q, zero weights skipped; a canonical"""
    acc = None
    for w, a in terms:
        if int(w) == 0:
            continue
        term = mulmod(a, int(w) % q, q)
        acc = term if acc is None else (acc + term) % np.uint64(q)      # both below q < 2^61: no wrap
    return acc


def block8x8_direct(q, X, L, R, pre=None, post=None):
    """X: uint64 [..., 64, size, k, n]; the same map evaluated residue by residue"""
    X = np.asarray(X, dtype=np.uint64)
    out = np.empty_like(X)
    for i, qi in enumerate(q):
        x = [[X[..., 8 * a + b, :, i, :] if pre is None else mulmod(X[..., 8 * a + b, :, i, :], int(pre[a][b]) % qi, qi) for b in range(8)] for a in range(8)]
        cols = [[_lin([(L[u][a], x[a][y]) for a in range(8)], qi) for y in range(8)] for u in range(8)]
        for u in range(8):
            for v in range(8):
                y = _lin([(R[v][b], cols[u][b]) for b in range(8)], qi)
                out[..., 8 * u + v, :, i, :] = y if post is None else mulmod(y, int(post[u][v]) % qi, qi)
    return out


def add_plain_constant(q, t, m):
    """what add_plain adds to coefficient 0 of c0 for the plaintext coefficient m in [0, t), per prime: Delta m, plus q mod t in the upper
    half (SEAL 2.3's preencrypt)"""
    Q = 1
    for qi in q:
        Q *= qi
    v = (Q // t) * m + (Q % t if m >= (t + 1) // 2 else 0)
    return [v % qi for qi in q]


def channel_mix_direct(q, t, M, planes, bias=None):
    """planes: uint64 [c, ..., size, k, n] -> [m, ..., size, k, n]"""
    planes = np.asarray(planes, dtype=np.uint64)
    M = np.asarray(M, dtype=np.int64)
    out = np.empty((M.shape[0],) + planes.shape[1:], dtype=np.uint64)
    for i, qi in enumerate(q):
        for o in range(M.shape[0]):
            out[o, ..., i, :] = _lin([(M[o][j], planes[j, ..., i, :]) for j in range(M.shape[1])], qi)
            if bias is not None and int(bias[o]) != 0:
                add = add_plain_constant(q, t, int(bias[o]) % t)[i]
                out[o, ..., 0, i, 0] = (out[o, ..., 0, i, 0] + np.uint64(add)) % np.uint64(qi)
    return out


# ---- the JPEG integer model and its float reference --------------------------------------------------------------------------------------
def float_dct_quant(blocks, quant):
    """round-half-away(float64 orthonormal 8x8 DCT-II / Q) of [..., 8, 8] level-shifted pixels"""
    u, x = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    D = np.where(u == 0, np.sqrt(0.5), 1.0) * 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    y = D @ np.asarray(blocks, dtype=np.float64) @ D.T / np.asarray(quant, dtype=np.float64).reshape(8, 8)
    return (np.sign(y) * np.floor(np.abs(y) + 0.5)).astype(np.int64)


def blocks8(channel):
    """[H, W] -> [H/8 * W/8, 8, 8] in raster order"""
    a = np.asarray(channel)
    h, w = a.shape
    return a.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
