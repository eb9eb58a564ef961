"""Op-by-op specification of the 2-D convolution filters (include/fhe_hip.h, fhe_filter2d) on any Evaluator-shaped object -- the CPU
oracle (one ciphertext [size][k][n] per call) or the GPU Evaluator (whole batches) -- and the same filter in floating point with the
same border rule.  Nothing here calls the library's own index arithmetic: tap_plan is an independent statement of the rule."""
import numpy as np

KERNELS = {
    # name: (weights [kh][kw], anchor (x, y), stride (x, y))
    "box3": (np.full((3, 3), 1.0 / 9.0), (1, 1), (1, 1)),
    "gauss3": (np.outer([1, 2, 1], [1, 2, 1]) / 16.0, (1, 1), (1, 1)),
    "gauss5": (np.outer([1, 4, 6, 4, 1], [1, 4, 6, 4, 1]) / 256.0, (2, 2), (1, 1)),
    "box7": (np.full((7, 7), 1.0 / 49.0), (3, 3), (1, 1)),
    "sobel_x": (np.array([[-1.0, 0, 1], [-2, 0, 2], [-1, 0, 1]]), (1, 1), (1, 1)),
    "sobel_y": (np.array([[-1.0, -2, -1], [0, 0, 0], [1, 2, 1]]), (1, 1), (1, 1)),
    "laplace": (np.array([[0.0, 1, 0], [1, -4, 1], [0, 1, 0]]), (1, 1), (1, 1)),
    "sharpen": (np.array([[0.0, -1, 0], [-1, 5, -1], [0, -1, 0]]), (1, 1), (1, 1)),
    "chroma420": (np.full((2, 2), 0.25), (0, 0), (2, 2)),
    "minus8x8": (np.full((8, 8), -1.0), (3, 3), (1, 1)),          # 64 taps of one weight: the longest lazy sum
}


def dst_size(src_w, src_h, stride):
    return -(-src_w // stride[0]), -(-src_h // stride[1])


def tap_plan(src_w, src_h, channels, kw, kh, anchor, stride, rows=None, src_row0=0):
    """[(rows) * dst_w * channels][kw * kh] record indices, clamp-to-edge, relative to a window that starts at source row src_row0"""
    dw, dh = dst_size(src_w, src_h, stride)
    r0, r1 = (0, dh) if rows is None else rows
    out = []
    for y in range(r0, r1):
        for x in range(dw):
            for c in range(channels):
                row = []
                for j in range(kh):
                    sy = min(max(y * stride[1] + j - anchor[1], 0), src_h - 1)
                    for i in range(kw):
                        sx = min(max(x * stride[0] + i - anchor[0], 0), src_w - 1)
                        row.append(((sy - src_row0) * src_w + sx) * channels + c)
                out.append(row)
    return np.array(out, dtype=np.int64).reshape(-1, kw * kh)


def source_rows(src_h, kh, anchor_y, stride_y, row0, row1):
    lo = min(max(row0 * stride_y - anchor_y, 0), src_h - 1)
    hi = min(max((row1 - 1) * stride_y + kh - 1 - anchor_y, 0), src_h - 1)
    return lo, hi - lo + 1


def filter_output(A, M, is_zero, src, taps_row, weights):
    """one output of the specification: src[i] -> ciphertext i; M(x, value) = multiply_plain by encode(value); is_zero(value): encode(value)
    is the zero plaintext (such positions are skipped)"""
    acc = None
    for p, w in enumerate(np.asarray(weights, dtype=np.float64).reshape(-1)):
        if is_zero(float(w)):
            continue
        term = M(src(int(taps_row[p])), float(w))
        acc = term if acc is None else A(acc, term)
    return acc


class OracleOps:
    def __init__(self, orc):
        self.orc, self._enc = orc, {}

    def enc(self, v):
        if v not in self._enc:
            self._enc[v] = self.orc.encode(v)
        return self._enc[v]

    def A(self, a, b):
        return self.orc.add(a, b)

    def M(self, a, v):
        return self.orc.multiply_plain(a, self.enc(v))

    def is_zero(self, v):
        return not np.any(self.enc(v))

    def output(self, src, taps_row, weights):
        """src: numpy [n_src][size][k][n]"""
        return filter_output(self.A, self.M, self.is_zero, lambda i: src[i], taps_row, weights)


def conv_float(img, weights, anchor, stride):
    """img [h][w] (or [h][w][c]) -> the float convolution with clamp-to-edge borders"""
    img = np.asarray(img, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    kh, kw = w.shape
    h, wd = img.shape[:2]
    dw, dh = dst_size(wd, h, stride)
    out = np.zeros((dh, dw) + img.shape[2:])
    for y in range(dh):
        for x in range(dw):
            for j in range(kh):
                sy = min(max(y * stride[1] + j - anchor[1], 0), h - 1)
                for i in range(kw):
                    sx = min(max(x * stride[0] + i - anchor[0], 0), wd - 1)
                    out[y, x] += w[j, i] * img[sy, sx]
    return out
