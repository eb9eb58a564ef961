"""Op-by-op compositions of the inverse JPEG steps (include/fhe_hip.h, fhe_idct8x8_dequant / fhe_ycc_to_rgb_blocks) on
any Evaluator-shaped object: the CPU oracle (one ciphertext [2][k][n] per call -- a stack of ciphertexts passed as one
array would be read as ONE ciphertext of that size) or the GPU Evaluator (whole batches [..., 2, k, n] per call)."""

IDCT_CONSTS = (0.541196100, 0.765366865, -1.847759065, 1.175875602, 0.298631336, 2.053119869,
               3.072711026, 1.501321110, -0.899976223, -2.562915447, -1.961570560, -0.390180644)


def idct_line(A, S, M, d):
    """the spec's idct_line: A = add, S = sub, M(x, value) = multiply_plain by encode(value)"""
    z1 = M(A(d[2], d[6]), 0.541196100)
    t2 = A(z1, M(d[6], -1.847759065))
    t3 = A(z1, M(d[2], 0.765366865))
    t0, t1 = A(d[0], d[4]), S(d[0], d[4])
    t10, t13, t11, t12 = A(t0, t3), S(t0, t3), A(t1, t2), S(t1, t2)
    u0, u1, u2, u3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = A(u0, u3), A(u1, u2), A(u0, u2), A(u1, u3)
    z5 = M(A(z3, z4), 1.175875602)
    u0, u1, u2, u3 = M(u0, 0.298631336), M(u1, 2.053119869), M(u2, 3.072711026), M(u3, 1.501321110)
    z1, z2 = M(z1, -0.899976223), M(z2, -2.562915447)
    z3, z4 = A(M(z3, -1.961570560), z5), A(M(z4, -0.390180644), z5)
    u0, u1, u2, u3 = A(u0, A(z1, z3)), A(u1, A(z2, z4)), A(u2, A(z2, z3)), A(u3, A(z1, z4))
    return [A(t10, u3), A(t11, u2), A(t12, u1), A(t13, u0), S(t13, u0), S(t12, u1), S(t11, u2), S(t10, u3)]


def idct_block(A, S, M, cts, quant=None):
    """steps 1-4 of fhe_idct8x8_dequant on a list of 64 ciphertexts (row-major); returns the 64 results"""
    c = list(cts)
    if quant is not None:
        c = [M(x, float(qv)) for x, qv in zip(c, quant)]
    for r in range(8):
        c[8 * r:8 * r + 8] = idct_line(A, S, M, c[8 * r:8 * r + 8])
    for col in range(8):
        out = idct_line(A, S, M, [c[col + 8 * i] for i in range(8)])
        for i in range(8):
            c[col + 8 * i] = out[i]
    return [M(x, 0.125) for x in c]


def ycc_to_rgb(A, S, M, AP, y, cb, cr):
    """JFIF inverse of rgb_to_ycc_fhe on one (Y, Cb, Cr) triple; AP(x, value) = add_plain of encode(value)"""
    y1 = AP(y, 128.0)
    r = A(y1, M(cr, 1.402))
    g = S(S(y1, M(cb, 0.344136)), M(cr, 0.714136))
    b = A(y1, M(cb, 1.772))
    return r, g, b


class OracleOps:
    """A / S / M / AP of the CPU oracle with the encodings cached"""

    def __init__(self, orc):
        self.orc, self._enc = orc, {}

    def enc(self, v):
        if v not in self._enc:
            self._enc[v] = self.orc.encode(v)
        return self._enc[v]

    def A(self, a, b):
        return self.orc.add(a, b)

    def S(self, a, b):
        return self.orc.sub(a, b)

    def M(self, a, v):
        return self.orc.multiply_plain(a, self.enc(v))

    def AP(self, a, v):
        return self.orc.add_plain(a, self.enc(v))

    def idct_block(self, block, quant=None):
        """block: [64][2][k][n] numpy; returns the same shape"""
        import numpy as np
        return np.stack(idct_block(self.A, self.S, self.M, [block[i] for i in range(64)], quant))

    def ycc_to_rgb_block(self, block):
        """block: [3][64][2][k][n] numpy (Y, Cb, Cr); returns [3][64][2][k][n] (R, G, B)"""
        import numpy as np
        out = np.empty_like(block)
        for i in range(64):
            out[0, i], out[1, i], out[2, i] = ycc_to_rgb(self.A, self.S, self.M, self.AP, block[0, i], block[1, i], block[2, i])
        return out


def fdct_float(x):
    """the forward 8x8 DCT the library's encrypted_dct + 0.125 scale computes (orthonormal JPEG DCT), in floating point"""
    import numpy as np
    k = np.arange(8)
    C = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) / 2
    C[0] /= np.sqrt(2)
    return C @ np.asarray(x, dtype=np.float64).reshape(8, 8) @ C.T
