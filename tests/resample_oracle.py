"""Independent statement of resampling with public weights (include/fhe_hip.h, fhe_remap / fhe_resample_axis_plan): the axis plans
(taps, weights, both coordinate conventions, antialias widths, weight_bits rounding) in plain Python floats, the op-by-op composition
of one remap output on any Evaluator-shaped object -- the CPU oracle (one ciphertext [size][k][n] per call) or the GPU Evaluator
(whole batches) --, the two-pass composition of a separable resize, and the same resample in float64 with the same weights.  Nothing
here calls the library's own index or weight arithmetic."""
import math

import numpy as np

SKIP = 0xFFFFFFFF
KERNELS = {"triangle": 0, "catmull_rom": 1, "reference_cubic": 2, "lanczos3": 3, "box": 4}
TWICE_RADIUS = {"triangle": 2, "catmull_rom": 4, "reference_cubic": 4, "lanczos3": 6, "box": 1}


def kernel_value(kernel, d):
    """the kernel at signed distance d = (tap position - sample position) / filter scale"""
    a = abs(d)
    if kernel == "triangle":
        return 1.0 - a if a < 1.0 else 0.0
    if kernel == "catmull_rom":
        if a <= 1.0:
            return (1.5 * a - 2.5) * a * a + 1.0
        if a < 2.0:
            return ((-0.5 * a + 2.5) * a - 4.0) * a + 2.0
        return 0.0
    if kernel == "reference_cubic":                    # Cubic() with t3 = t * t: (t^2 - t) / 2, 1 - t^2, (t^2 + t) / 2, 0 at taps -1, 0, 1, 2
        if d <= -2.0 or d > 1.0:
            return 0.0
        if d <= -1.0:
            t = -1.0 - d
            return (t * t - t) / 2.0
        if d <= 0.0:
            t = -d
            return 1.0 - t * t
        t = 1.0 - d
        return (t * t + t) / 2.0
    if kernel == "lanczos3":
        if a >= 3.0:
            return 0.0
        if a == 0.0:
            return 1.0
        px = math.pi * d
        return 3.0 * math.sin(px) * math.sin(px / 3.0) / (px * px)
    if kernel == "box":
        return 1.0 if -0.5 <= d < 0.5 else 0.0
    raise KeyError(kernel)


def reference_coordinate(x, dst_len, src_len):
    """float u = float(x) / float(dst_len - 1) * float(src_len) - 0.5 (the product in float32, the shift in double, the store in float32)"""
    f = np.float32
    return f(float(f(f(f(x) / f(dst_len - 1)) * f(src_len))) - 0.5)


def axis_width(src_len, dst_len, kernel, antialias=False, convention="half_pixel"):
    if convention == "half_pixel" and src_len == dst_len:
        return 1
    r2 = TWICE_RADIUS[kernel]
    if antialias and src_len > dst_len:
        c = -(-(r2 * src_len) // (2 * dst_len))        # ceil(radius * src / dst)
    else:
        c = (r2 + 1) // 2
    return 2 * c


def axis_plan(src_len, dst_len, kernel, antialias=False, convention="half_pixel", weight_bits=None):
    """(taps int64 [dst_len][T], weights float64 [dst_len][T])"""
    T = axis_width(src_len, dst_len, kernel, antialias, convention)
    if T > 64:
        raise ValueError("more than 64 taps")
    taps = np.zeros((dst_len, T), dtype=np.int64)
    weights = np.zeros((dst_len, T), dtype=np.float64)
    if convention == "half_pixel" and src_len == dst_len:
        taps[:, 0] = np.arange(dst_len)
        weights[:, 0] = 1.0
        return taps, weights
    c = T // 2
    fs = float(src_len) / float(dst_len) if (antialias and src_len > dst_len) else 1.0
    for x in range(dst_len):
        if convention == "half_pixel":
            u = (float(x) + 0.5) * float(src_len) / float(dst_len) - 0.5
            first = math.floor(u) - c + 1
            dist = [float(first + i) - u for i in range(T)]
        else:
            uf = reference_coordinate(x, dst_len, src_len)
            first = int(uf) - c + 1                    # int(): towards zero
            off = float(np.float32(uf - np.float32(math.floor(uf))))
            dist = [float(i - c + 1) - off for i in range(T)]
        w = [kernel_value(kernel, d / fs) for d in dist]
        total = 0.0
        for v in w:
            total += v
        w = [v / total for v in w]
        if weight_bits:
            S = float(1 << weight_bits)
            m = [int(math.floor(v * S + 0.5)) for v in w]
            big = 0
            for i in range(T):
                if w[i] > w[big]:
                    big = i
            m[big] += (1 << weight_bits) - sum(m)
            w = [mi / S for mi in m]
        taps[x] = [min(max(first + i, 0), src_len - 1) for i in range(T)]
        weights[x] = w
    return taps, weights


# ---- the specification of one output, and of the two-pass resize --------------------------------------------------------------------
def remap_output(A, M, is_zero, src, taps_row, wids_row, values):
    """one output of fhe_remap's specification: src(i) -> ciphertext i; M(x, value) = multiply_plain by encode(value); is_zero(value):
    encode(value) is the zero plaintext"""
    acc = None
    for p in range(len(taps_row)):
        if int(wids_row[p]) == SKIP:
            continue
        v = float(values[int(wids_row[p])])
        if is_zero(v):
            continue
        term = M(src(int(taps_row[p])), v)
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

    def output(self, src, taps_row, wids_row, values):
        """src: numpy [n_src][size][k][n], or a callable index -> ciphertext"""
        get = src if callable(src) else (lambda i: src[i])
        return remap_output(self.A, self.M, self.is_zero, get, taps_row, wids_row, values)

    def weighted(self, src, taps_row, weights_row):
        """the same with the weights given per slot"""
        return self.output(src, taps_row, list(range(len(taps_row))), weights_row)


def resize_output(ops, src, src_w, channels, plan_x, plan_y, x, y, ch=0, order="hv"):
    """Output pixel (x, y), channel ch of the two-pass resize, op by op: "hv" = horizontal pass first (the specification), "vh" = vertical
    first.  src: [src_h * src_w * channels][size][k][n] records.  plan_x, plan_y: (taps, weights) of the axes."""
    (tx, wx), (ty, wy) = plan_x, plan_y
    memo = {}
    if order == "hv":
        def mid(row):                                  # the horizontally resampled pixel (x, row)
            if row not in memo:
                memo[row] = ops.weighted(lambda i: src[(row * src_w + i) * channels + ch], tx[x], wx[x])
            return memo[row]
        return ops.weighted(mid, ty[y], wy[y])

    def mid(col):                                      # the vertically resampled pixel (col, y)
        if col not in memo:
            memo[col] = ops.weighted(lambda j: src[(j * src_w + col) * channels + ch], ty[y], wy[y])
        return memo[col]
    return ops.weighted(mid, tx[x], wx[x])


def resample_float(img, plan_x, plan_y):
    """img [h][w] (or [h][w][c]) -> the float64 separable resample with the plans' taps and weights, horizontal pass first"""
    img = np.asarray(img, dtype=np.float64)
    (tx, wx), (ty, wy) = plan_x, plan_y
    mid = np.zeros((img.shape[0], tx.shape[0]) + img.shape[2:])
    for p in range(tx.shape[1]):
        mid += img[:, tx[:, p]] * wx[:, p].reshape((1, -1) + (1,) * (img.ndim - 2))
    out = np.zeros((ty.shape[0], tx.shape[0]) + img.shape[2:])
    for p in range(ty.shape[1]):
        out += mid[ty[:, p]] * wy[:, p].reshape((-1, 1) + (1,) * (img.ndim - 2))
    return out
