"""The reference's homomorphic circuits on whole batches: ctypes callers of include/fhe_circuits.h.

The circuits themselves -- tap gathers, the t^2 reuse of Cubic, prepared operands, the growth of ciphertext
sizes, every temporary -- live inside libfhe_hip.so (csrc/circuits.hip); this module only allocates the
output and scratch tensors and passes pointers, so a C++ host gets exactly the same batched path
(seal/hip_circuits.h).  The leading dimension of every ciphertext tensor ([B, size, k, n]) runs over
independent pixels / output positions, which the reference visits in serial loops
(homo/server_jpeg.cpp:113, homo/fhe_resize.h:350,381, homo/server_decode.cpp:120-137).

Server-side fresh encryptions inside the reference's circuits (the fractional offsets in
SampleLinear/SampleBicubic, homo/fhe_resize.h:230-266, and the Enc(0) accumulators of
homomorphic_sin/cos, homo/fhe_decode.h:54,134) are randomised; here they are explicit inputs so that
results are reproducible.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .evaluator import YQT, Block8x8Plan, FractionalEncoder, PlaneMapPlan, PreparedPlain, _ptr, _stream, check_evaluation_keys


class PlainCache:
    """encode + lift + NTT each distinct constant once (the reference redoes it on every call)."""

    def __init__(self, ctx, encoder=None):
        self.ctx = ctx
        self.enc = encoder or FractionalEncoder(ctx)
        self._prepared = {}
        self._plain = {}

    def plain(self, v):
        v = float(v)
        if v not in self._plain:
            self._plain[v] = self.enc.encode(v)
        return self._plain[v]

    def prepared(self, v):
        v = float(v)
        if v not in self._prepared:
            self._prepared[v] = PreparedPlain(self.ctx, self.plain(v))
        return self._prepared[v]


# ------------------------------------------------------------------------------------------------
# JPEG path, op-at-a-time (the fused kernel is Evaluator.dct8x8_quant)
# ------------------------------------------------------------------------------------------------
def rgb_to_ycc(ev, pc, r, g, b):
    """homo/fhe_image.h:310-325 as separate Evaluator calls (fused form: Evaluator.rgb_to_ycc)."""
    M, P = ev.multiply_plain, pc.prepared
    y = ev.sub_plain(ev.add(ev.add(M(r, P(0.299)), M(g, P(0.587))), M(b, P(0.114))), pc.plain(128.0))
    u = ev.add(ev.sub(M(r, P(-0.168736)), M(g, P(0.331264))), M(b, P(0.5)))
    v = ev.sub(ev.sub(M(r, P(0.5)), M(g, P(0.418688))), M(b, P(0.081312)))
    return y, u, v


# ------------------------------------------------------------------------------------------------
# the circuits handle and scratch
# ------------------------------------------------------------------------------------------------
CUBIC, LINEAR, SAMPLE_BICUBIC, SAMPLE_LINEAR, SINCOS, STEP, DECODE = range(7)      # FHE_CIRC_* of include/fhe_circuits.h


class Circuits:
    """fhe_circuits: the constants of the resize / decode circuits for one context and encoder.
    relin=(evk_ntt, dbc): the RELINEARISED mode (fhe_circuits_create_relin; SURVEY.md section 8(f) #4, not what the
    reference does): evaluator.relinearize after every multiply / square, so every ciphertext of every circuit has two
    polynomials.  evk_ntt as KeyGenerator.generate_evaluation_keys(dbc) returns it; the handle keeps it alive.
    relin=(evk_ntt, dbc, "cubic"): the second placement (FHE_RELIN_PER_CUBIC, include/fhe_circuits.h): the reference's Cubic /
    Linear sequences unchanged and ONE relinearize at the end of each (size 4 / 3 -> 2; two key switches per Cubic where the
    first placement spends five); evk_ntt = generate_evaluation_keys(dbc, 2): the keys for s^2 and s^3.  Resize circuits only.
    relin=(evk_ntt, dbc, "sample"): the third (FHE_RELIN_PER_SAMPLE): the samplers exactly as the reference evaluates them and ONE relinearize of
    every output pixel (6 -> 2 / 4 -> 2); evk_ntt = generate_evaluation_keys(dbc, 4): the keys for s^2 .. s^5.  Resize circuits only."""

    def __init__(self, ctx, int_coeffs=100, frac_coeffs=100, relin=None):
        self.ctx = ctx
        h = C.c_void_p()
        if relin is None:
            _lib.call("fhe_circuits_create", ctx.h, int_coeffs, frac_coeffs, C.byref(h))
        else:
            self._evk, dbc = relin[0], relin[1]
            placement = relin_placement(relin)
            check_evaluation_keys(ctx, self._evk, dbc, (1, 2, 4)[placement], "Circuits")
            if placement == 1:
                assert self._evk.dim() == 6 and self._evk.shape[0] >= 2, "per-Cubic placement: keys for s^2 and s^3 (generate_evaluation_keys(dbc, 2))"
            if placement == 2:
                assert self._evk.dim() == 6 and self._evk.shape[0] >= 4, "per-sample placement: keys for s^2 .. s^5 (generate_evaluation_keys(dbc, 4))"
            _lib.call("fhe_circuits_create_relin_at", ctx.h, int_coeffs, frac_coeffs, _ptr(self._evk), int(dbc), placement, C.byref(h))
        self.h = h
        self._scratch = None

    def out_size(self, circuit, arg=0):
        return int(_lib.load().fhe_circuits_out_size(self.h, circuit, arg))

    def __del__(self):
        h = getattr(self, "h", None)
        if h:
            try:
                _lib.load().fhe_circuits_destroy(h)
            except Exception:
                pass
            self.h = None

    def scratch(self, nbytes):
        if not nbytes:
            raise _lib.FheError(-1, _lib.load().fhe_last_error().decode("utf-8", "replace") or "scratch query failed")
        if self._scratch is None or self._scratch.numel() < nbytes:
            self._scratch = None
            self._scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.ctx.device)
        return self._scratch


def relin_placement(relin):
    """0: after every product (relin=(evk, dbc)), 1: once per Cubic / Linear (relin=(evk, dbc, "cubic"))"""
    if relin is None or len(relin) < 3 or relin[2] in (0, None, "product", "every"):
        return 0
    if relin[2] in (1, "cubic"):
        return 1
    if relin[2] in (2, "sample"):
        return 2
    raise ValueError("relin placement must be 'product', 'cubic' or 'sample', got %r" % (relin[2],))


def circuits_of(pc, relin=None):
    """the fhe_circuits handle that goes with a PlainCache (same context and encoder), created on first use;
    relin=(evk_ntt, dbc): the relinearising handle for those keys"""
    if relin is not None:
        cache = pc.__dict__.setdefault("_circuits_relin", {})
        key = (relin[0].data_ptr(), int(relin[1]), relin_placement(relin))
        if key not in cache:
            cache[key] = Circuits(pc.ctx, pc.enc.int_coeffs, pc.enc.frac_coeffs, relin=relin)
        return cache[key]
    h = getattr(pc, "_circuits", None)
    if h is None:
        h = pc._circuits = Circuits(pc.ctx, pc.enc.int_coeffs, pc.enc.frac_coeffs)
    return h


def _count(t, size):
    assert t.dtype == torch.int64 and t.is_contiguous() and t.shape[-3] == size, (t.shape, size)
    c = 1
    for d in t.shape[:-3]:
        c *= d
    return c


def _taps_array(taps, width):
    a = np.ascontiguousarray(taps, dtype=np.uint32)
    assert a.ndim == 2 and a.shape[1] == width, a.shape
    return a


# ------------------------------------------------------------------------------------------------
# resize path
# ------------------------------------------------------------------------------------------------
def _base2_cubic_constants(pc):
    """True if the encoder writes Cubic's constants the way the fused passes assume (base 2):
    encode(3) = x+1, encode(2) = x, encode(5) = x^2+1, encode(4) = x^2, encode(0.5) = -x^(n-1)."""
    t, n = pc.ctx.t, pc.ctx.n

    def nz(v):
        p = np.asarray(pc.plain(v), dtype=np.uint64)
        return {int(i): int(p[i]) for i in np.nonzero(p)[0]}

    return (nz(3) == {0: 1, 1: 1} and nz(2) == {1: 1} and nz(5) == {0: 1, 2: 1} and nz(4) == {2: 1}
            and nz(0.5) == {n - 1: t - 1})


def cubic_evaluator_calls(ev, pc, A, B, C, D, t, relin=None):
    """Cubic(result, A,B,C,D,t) as the reference's Evaluator call sequence, one (batched) call per line of
    homo/fhe_resize.h:149-188 -- the op-by-op form the fused circuit (cubic below) is tested against, and the
    carrier of the relinearised mode: relin=(evk_ntt, dbc) brings every product back to size 2 (SURVEY.md
    section 8(f) #4, NOT what the reference does), so the result has size 2 instead of s+2; ciphertext bits
    then differ from the reference path by construction (key-switching noise), the decrypted value does not."""
    M, P = ev.multiply_plain, pc.prepared
    each = relin is not None and relin_placement(relin) == 0     # relinearize after every product
    tail = relin is not None and relin_placement(relin) in (1, 2)    # the reference's sequence, ONE relinearize of the result (relin=(evk, dbc, "cubic"); a
    #                                                                  stand-alone Cubic of the "sample" placement is relinearised by its caller the same way)

    def mul(x, y):
        z = ev.multiply(x, y)
        return ev.relinearize(z, relin[0], relin[1]) if each and z.shape[-3] == 3 else z

    a = ev.add(ev.sub(ev.sub(M(B, P(3)), A), M(C, P(3))), D)
    b = ev.sub(ev.add(ev.sub(M(A, P(2)), M(B, P(5))), M(C, P(4))), D)
    c = ev.sub(C, A)
    t2 = ev.square(t)
    if each and t2.shape[-3] == 3:
        t2 = ev.relinearize(t2, relin[0], relin[1])
    t3 = t2 if each else ev.multiply(t, t)                       # t3 = t * t exactly as the reference computes it (:175)
    a, b, c = mul(a, t3), mul(b, t2), mul(c, t)
    a = ev.add(ev.add(a, b), c)
    a = M(a, P(0.5))
    a = ev.add(a, B)
    return ev.relinearize(a, relin[0], relin[1]) if tail else a


def cubic(ev, pc, A, B, C, D, t, relin=None):
    """Cubic(result, A,B,C,D,t): homo/fhe_resize.h:143-189 for a batch (fhe_cubic).  Note t3 = t*t exactly as the
    reference computes it (:175).  relin=(evk_ntt, dbc) selects the relinearised mode of the library (every product
    relinearised: result of size 2); cubic_evaluator_calls(..., relin) is the same thing one Evaluator call at a time."""
    cc = circuits_of(pc, relin)
    size = A.shape[-3]
    count = _count(A, size)
    assert A.shape == B.shape == C.shape == D.shape and _count(t, 2) == count
    out = ev.ctx.empty(*A.shape[:-3], size=cc.out_size(CUBIC, size))
    nbytes = _lib.load().fhe_cubic_scratch_bytes(cc.h, size, count)
    scr = cc.scratch(nbytes)
    _lib.call("fhe_cubic", cc.h, _ptr(A), _ptr(B), _ptr(C), _ptr(D), size, _ptr(t), _ptr(out), count, _ptr(scr), nbytes, _stream())
    return out


def linear(ev, pc, A, B, t, relin=None):
    """Linear(result, A,B,t): homo/fhe_resize.h:191-204: (1 - t) A + t B (fhe_linear)."""
    cc = circuits_of(pc, relin)
    size = A.shape[-3]
    count = _count(A, size)
    assert A.shape == B.shape and _count(t, 2) == count
    out = ev.ctx.empty(*A.shape[:-3], size=cc.out_size(LINEAR, size))
    nbytes = _lib.load().fhe_linear_scratch_bytes(cc.h, size, count)
    scr = cc.scratch(nbytes)
    _lib.call("fhe_linear", cc.h, _ptr(A), _ptr(B), size, _ptr(t), _ptr(out), count, _ptr(scr), nbytes, _stream())
    return out


def resize_sample_plan(src_w, src_h, dst_w, dst_h, bicubic=True):
    """The index arithmetic of ResizeImage / SampleBicubic / SampleLinear / GetPixelClamped
    (homo/fhe_resize.h:350-351, 381-382, 260-290, 215-220), in float32 like the reference
    (fhe_resize_sample_plan).  Returns per output pixel: the clamped source pixel indices (uint32 array
    [dst_w * dst_h, 16] for bicubic, row-major 4x4; [.., 4] for bilinear) and the fractional offsets
    (xfract, yfract) as lists of floats."""
    npx = dst_w * dst_h
    taps = np.zeros((npx, 16 if bicubic else 4), dtype=np.uint32)
    fx, fy = np.zeros(npx), np.zeros(npx)
    _lib.call("fhe_resize_sample_plan", src_w, src_h, dst_w, dst_h, int(bool(bicubic)), taps.ctypes.data_as(C.c_void_p),
              fx.ctypes.data_as(C.c_void_p), fy.ctypes.data_as(C.c_void_p))
    return taps, [float(v) for v in fx], [float(v) for v in fy]


def _sample(name, width, kind, ev, pc, pixels, taps, xfract, yfract, relin=None):
    cc = circuits_of(pc, relin)
    out_size = cc.out_size(kind)
    taps = _taps_array(taps, width)
    count = taps.shape[0]
    n_pixels = _count(pixels, 2)
    assert _count(xfract, 2) == count and _count(yfract, 2) == count
    out = ev.ctx.empty(count, size=out_size)
    L = _lib.load()
    nbytes = getattr(L, name + "_scratch_bytes")(cc.h, count)
    scr = cc.scratch(nbytes)
    _lib.call(name, cc.h, _ptr(pixels), n_pixels, taps.ctypes.data_as(C.c_void_p), _ptr(xfract), _ptr(yfract), _ptr(out), count,
              _ptr(scr), nbytes, _stream())
    return out


def sample_bicubic(ev, pc, pixels, taps, xfract, yfract, relin=None):
    """SampleBicubic for a batch of output pixels and one colour channel (homo/fhe_resize.h:254-305;
    fhe_sample_bicubic).  pixels: [src_pixels, 2, k, n]; taps: [B][16] source indices; xfract/yfract: [B, 2, k, n]
    ciphertexts of the fractional offsets.  Returns [B, 6, k, n] ([B, 2, k, n] with relin=(evk_ntt, dbc))."""
    return _sample("fhe_sample_bicubic", 16, SAMPLE_BICUBIC, ev, pc, pixels, taps, xfract, yfract, relin)


def sample_linear(ev, pc, pixels, taps, xfract, yfract, relin=None):
    """SampleLinear for one channel (homo/fhe_resize.h:222-252; fhe_sample_linear).  Returns [B, 4, k, n] ([B, 2, k, n] relinearised)."""
    return _sample("fhe_sample_linear", 4, SAMPLE_LINEAR, ev, pc, pixels, taps, xfract, yfract, relin)


# ------------------------------------------------------------------------------------------------
# 2-D convolution filters (Evaluator.filter2d / fhe_filter2d)
# ------------------------------------------------------------------------------------------------
def _filter(weights, anchor=None, stride=(1, 1)):
    w = np.array(weights, dtype=np.float64)
    return dict(weights=w, anchor=filter_anchor(w.shape[1], w.shape[0]) if anchor is None else anchor, stride=stride)


def filter_anchor(kw, kh):
    """default anchor of a kw x kh kernel: its centre, the upper-left of the four central positions for even extents"""
    return ((kw - 1) // 2, (kh - 1) // 2)


# named kernels: weights [kh][kw], anchor (x, y), stride (x, y)
FILTERS = {
    "box3": _filter(np.full((3, 3), 1.0 / 9.0)),
    "gauss3": _filter(np.outer([1, 2, 1], [1, 2, 1]) / 16.0),
    "gauss5": _filter(np.outer([1, 4, 6, 4, 1], [1, 4, 6, 4, 1]) / 256.0),
    "sobel_x": _filter([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]]),
    "sobel_y": _filter([[-1, -2, -1], [0, 0, 0], [1, 2, 1]]),
    "laplace": _filter([[0, 1, 0], [1, -4, 1], [0, 1, 0]]),
    "sharpen": _filter([[0, -1, 0], [-1, 5, -1], [0, -1, 0]]),
    "chroma420": _filter(np.full((2, 2), 0.25), anchor=(0, 0), stride=(2, 2)),      # the 2x2 average of 4:2:0 chroma subsampling
}


def filter_tap_plan(src_w, src_h, kw, kh, channels=1, anchor=None, stride=(1, 1), rows=None, src_row0=None, taps=True):
    """Index arithmetic of a kw x kh filter with clamp-to-edge borders (fhe_filter_tap_plan): returns (taps, dst_w, dst_h), taps a
    uint32 array [(row1 - row0) * dst_w * channels][kw * kh] of record indices for destination rows `rows` (default: all), relative to a
    resident window that starts at source row `src_row0` (default: the first row those destination rows read).  Record of pixel
    (x, y), channel c: (y * src_w + x) * channels + c; outputs in the same interleaved order.  taps=False only reports the sizes."""
    ax, ay = filter_anchor(kw, kh) if anchor is None else anchor
    sx, sy = stride
    dw, dh = C.c_uint32(), C.c_uint32()
    _lib.call("fhe_filter_tap_plan", src_w, src_h, channels, kw, kh, ax, ay, sx, sy, 0, 0, 0, C.byref(dw), C.byref(dh), None)
    dst_w, dst_h = int(dw.value), int(dh.value)
    if not taps:
        return None, dst_w, dst_h
    row0, row1 = (0, dst_h) if rows is None else (int(rows[0]), int(rows[1]))
    if not (0 <= row0 < row1 <= dst_h):
        raise ValueError("rows %r are not a range of the %d destination rows" % (rows, dst_h))
    if src_row0 is None:
        src_row0 = filter_source_rows(src_h, kh, ay, sy, row0, row1)[0]
    out = np.zeros(((row1 - row0) * dst_w * channels, kw * kh), dtype=np.uint32)
    _lib.call("fhe_filter_tap_plan", src_w, src_h, channels, kw, kh, ax, ay, sx, sy, row0, row1, int(src_row0), C.byref(dw), C.byref(dh),
              out.ctypes.data_as(C.c_void_p))
    return out, dst_w, dst_h


def filter_source_rows(src_h, kh, anchor_y, stride_y, row0, row1):
    """(first, count) of the source rows destination rows [row0, row1) of a filter read (fhe_filter_source_rows): the rows plus the halo,
    clamped -- what a GPU that owns those destination rows has to load."""
    first, count = C.c_uint32(), C.c_uint32()
    _lib.call("fhe_filter_source_rows", src_h, kh, anchor_y, stride_y, row0, row1, C.byref(first), C.byref(count))
    return int(first.value), int(count.value)


# ------------------------------------------------------------------------------------------------
# Resampling with public weights (Evaluator.remap / fhe_remap)
# ------------------------------------------------------------------------------------------------
RESAMPLE_KERNELS = {"triangle": 0, "catmull_rom": 1, "reference_cubic": 2, "lanczos3": 3, "box": 4}      # FHE_RESAMPLE_* in include/fhe_hip.h
RESAMPLE_CONVENTIONS = {"half_pixel": 0, "reference": 1}


def resample_axis_plan(src_len, dst_len, kernel="catmull_rom", antialias=False, convention="half_pixel", weight_bits=None):
    """Index and weight arithmetic of one axis of a separable resize (fhe_resample_axis_plan, host only): returns (taps, weights), a
    uint32 and a float64 array [dst_len][T].  Output x is the sum over p of weights[x][p] * source[taps[x][p]]; taps are clamped to the
    edge, the weights of one output sum to 1 (exactly, as multiples of 2^-weight_bits, when weight_bits is given)."""
    k = RESAMPLE_KERNELS[kernel] if isinstance(kernel, str) else int(kernel)
    cv = RESAMPLE_CONVENTIONS[convention] if isinstance(convention, str) else int(convention)
    bits = 0 if weight_bits is None else int(weight_bits)
    T = C.c_uint32()
    _lib.call("fhe_resample_axis_plan", src_len, dst_len, k, int(bool(antialias)), cv, bits, C.byref(T), None, None)
    taps = np.zeros((dst_len, int(T.value)), dtype=np.uint32)
    weights = np.zeros((dst_len, int(T.value)), dtype=np.float64)
    _lib.call("fhe_resample_axis_plan", src_len, dst_len, k, int(bool(antialias)), cv, bits, C.byref(T), taps.ctypes.data_as(C.c_void_p),
              weights.ctypes.data_as(C.c_void_p))
    return taps, weights


def _weight_ids(weights):
    """weights [count][T] -> (values, wids): the distinct values and, per slot, the index of its value"""
    values, inverse = np.unique(weights, return_inverse=True)
    return values, inverse.reshape(weights.shape).astype(np.uint32)


def resize_plan(src_w, src_h, dst_w, dst_h, kernel="catmull_rom", channels=1, antialias=False, convention="half_pixel", weight_bits=None, rows=None,
                order=None):
    """The two Evaluator.remap passes of a separable resize with public weights, for destination rows `rows` (default: all).  Returns a
    dict: "source_rows" = (first, count), the source rows those destination rows read -- the caller hands Evaluator.resize_plain the
    records of exactly these rows, record of pixel (x, y), channel c at ((y - first) * src_w + x) * channels + c --; "passes" = two dicts
    (axis, taps [count][T], wids [count][T], values: the pass's weight table, count); "order"; "dst" = (dst_w, rows in the shard).
    The specification is "horizontal, then vertical" (order="hv"); the two passes commute as ring maps and give the same bits in either
    order, so by default the axis that leaves the smaller intermediate runs first (the vertical one when both leave the same)."""
    tx, wx = resample_axis_plan(src_w, dst_w, kernel, antialias, convention, weight_bits)
    ty, wy = resample_axis_plan(src_h, dst_h, kernel, antialias, convention, weight_bits)
    row0, row1 = (0, dst_h) if rows is None else (int(rows[0]), int(rows[1]))
    if not (0 <= row0 < row1 <= dst_h):
        raise ValueError("rows %r are not a range of the %d destination rows" % (rows, dst_h))
    ty, wy = ty[row0:row1].astype(np.int64), wy[row0:row1]
    tx = tx.astype(np.int64)
    live_y = wy != 0.0
    first = int(ty[live_y].min()) if np.any(live_y) else int(ty.min())
    last = int(ty[live_y].max()) if np.any(live_y) else int(ty.max())
    n_rows, out_rows = last - first + 1, row1 - row0
    ty = np.clip(ty - first, 0, n_rows - 1)            # slots of weight zero may point outside the window: they are never read
    if order is None:
        order = "hv" if n_rows * dst_w < out_rows * src_w else "vh"         # equal sizes: vertical first measured 0-1 % slower (128 -> 64) and 2-5 % faster (64 -> 128)
    if order not in ("hv", "vh"):
        raise ValueError("order must be 'hv', 'vh' or None, got %r" % (order,))
    ch = np.arange(channels, dtype=np.int64)

    def horizontal(n_lines):
        """[n_lines][src_w][channels] -> [n_lines][dst_w][channels]"""
        line = np.arange(n_lines, dtype=np.int64)
        taps = (line[:, None, None, None] * src_w + tx[None, :, None, :]) * channels + ch[None, None, :, None]
        values, wid = _weight_ids(wx)
        wids = np.broadcast_to(wid[None, :, None, :], taps.shape)
        return dict(axis="x", taps=taps.reshape(-1, tx.shape[1]).astype(np.uint32), wids=np.ascontiguousarray(wids).reshape(-1, tx.shape[1]), values=values)

    def vertical(width):
        """[n_rows][width][channels] -> [out_rows][width][channels]"""
        col = np.arange(width, dtype=np.int64)
        taps = (ty[:, None, None, :] * width + col[None, :, None, None]) * channels + ch[None, None, :, None]
        values, wid = _weight_ids(wy)
        wids = np.broadcast_to(wid[:, None, None, :], taps.shape)
        return dict(axis="y", taps=taps.reshape(-1, ty.shape[1]).astype(np.uint32), wids=np.ascontiguousarray(wids).reshape(-1, ty.shape[1]), values=values)

    passes = [horizontal(n_rows), vertical(dst_w)] if order == "hv" else [vertical(src_w), horizontal(out_rows)]
    for p in passes:
        p["count"] = int(p["taps"].shape[0])
    return dict(source_rows=(first, n_rows), passes=passes, order=order, dst=(dst_w, out_rows), src_w=src_w, channels=channels)


BAND_CONSUMER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p)


def resize_source_rows(src_h, dst_h, row0, row1, bicubic=True):
    """(first, count) of the source rows destination rows [row0, row1) read (fhe_resize_source_rows): the shard's rows plus
    the sampler's halo, clamped -- what a GPU that owns those destination rows has to load."""
    first, count = C.c_uint32(), C.c_uint32()
    _lib.call("fhe_resize_source_rows", src_h, dst_h, row0, row1, int(bool(bicubic)), C.byref(first), C.byref(count))
    return int(first.value), int(count.value)


def resize_bicubic_shared(ev, pc, pixels, src_w, src_h, dst_w, dst_h, xfract, yfract, batch=256, band_rows=4, consume=None, rows=None, src_rows=None,
                          relin=None):
    """ResizeImage with SampleBicubic (homo/fhe_resize.h:254-392) for one colour channel when the fractional
    offsets arrive as ONE ciphertext per output column (xfract [dst_w, 2, k, n]) and ONE per output row
    (yfract [dst_h, 2, k, n]) -- SURVEY.md section 8(d), config 3: "xfract/yfract ciphertexts are inputs generated
    per distinct fractional value" (fhe_resize_bicubic_shared).  frac(u) depends on x only and frac(v) on y only
    (:351,382), so with shared ciphertexts the reference's per-pixel work repeats itself and the library forms every
    repeated ring element once; each output equals sample_bicubic(..., xfract[x], yfract[y]) bit for bit:

      * a row Cubic (:296-299) is a function of (output column x, source row r) only; consecutive output rows'
        4-row windows overlap, so the 4 * dst_h row Cubics of a column collapse to one per source row touched
        (128 instead of 256 for 128 -> 64);
      * xfract^2 and the prepared (extended + transformed) forms of xfract, xfract^2 are formed once per column,
        yfract^2 and its prepared forms once per row; the products index them in place.

    The reference's server encrypts fresh offsets for every sample (:262,266); its results are therefore
    randomised per pixel and only sample_bicubic with per-pixel ciphertexts reproduces that run bit for bit
    (server.server_resize does).  Source rows are visited as a sliding window (`band_rows` output rows at a
    time), like the reference's loader (:352-379).

    rows=(y0, y1) evaluates a SHARD of the destination rows (fhe_resize_bicubic_shared_rows; the multi-GPU partition of
    the outer loop, :350): `pixels` then holds the source rows src_rows=(first, count) only (resize_source_rows: the
    shard's rows +- the halo), yfract the offsets of rows [y0, y1) only, and the result the pixels of those rows -- each
    bit-identical to the whole-image call's.

    relin=(evk_ntt, dbc): the relinearised mode (every product relinearised; outputs of size 2 instead of 6).

    Returns [dst_h * dst_w, 6, k, n] (row-major; [(y1 - y0) * dst_w, ...] for a shard), or None when
    `consume(first_pixel, tensor)` takes the bands (first_pixel is the global index y * dst_w; the tensor is a view of a
    buffer the library reuses: clone what must outlive the callback)."""
    cc = circuits_of(pc, relin)
    so = cc.out_size(SAMPLE_BICUBIC)
    ctx = ev.ctx
    y0, y1 = rows if rows is not None else (0, dst_h)
    s0, sc = src_rows if src_rows is not None else ((0, src_h) if rows is None else resize_source_rows(src_h, dst_h, y0, y1))
    assert _count(pixels, 2) == src_w * sc and _count(xfract, 2) == dst_w and _count(yfract, 2) == y1 - y0, (pixels.shape, sc, yfract.shape, rows)
    L = _lib.load()
    out = None if consume is not None else ctx.empty(dst_w * (y1 - y0), size=so)
    nbytes = L.fhe_resize_bicubic_shared_rows_scratch_bytes(cc.h, src_w, src_h, dst_w, dst_h, y0, y1, s0, sc, batch, band_rows, int(out is not None))
    scr = cc.scratch(nbytes)
    words = so * ctx.k * ctx.n
    err = []

    def on_band(_user, first, d_band, npx, _stream_):
        try:
            off = d_band - scr.data_ptr()                              # the band buffer lies inside the scratch tensor
            assert 0 <= off and off + npx * words * 8 <= scr.numel() and off % 8 == 0
            consume(int(first), scr[off:off + npx * words * 8].view(torch.int64).view(npx, so, ctx.k, ctx.n))
            return 0
        except BaseException as e:                                     # must not propagate through the C frame
            err.append(e)
            return -1

    cb = BAND_CONSUMER(on_band) if consume is not None else None
    try:
        _lib.call("fhe_resize_bicubic_shared_rows", cc.h, _ptr(pixels), src_w, src_h, dst_w, dst_h, y0, y1, s0, sc, _ptr(xfract), _ptr(yfract),
                  _ptr(out) if out is not None else C.c_void_p(None), batch, band_rows, cb, None, _ptr(scr), nbytes, _stream())
    except _lib.FheError:
        if err:
            raise err[0]
        raise
    return out


# ------------------------------------------------------------------------------------------------
# decode path
# ------------------------------------------------------------------------------------------------
def _sincos(cosine, ev, pc, x, zero, relin=None):
    cc = circuits_of(pc, relin)
    count = _count(x, 2)
    assert _count(zero, 2) == count
    out = ev.ctx.empty(*x.shape[:-3], size=cc.out_size(SINCOS))
    nbytes = _lib.load().fhe_homomorphic_sincos_scratch_bytes(cc.h, count)
    scr = cc.scratch(nbytes)
    _lib.call("fhe_homomorphic_sincos", cc.h, cosine, _ptr(x), _ptr(zero), _ptr(out), count, _ptr(scr), nbytes, _stream())
    return out


def homomorphic_sin(ev, pc, x, zero, relin=None):
    """homo/fhe_decode.h:48-120; `zero` plays the role of encrypt(encode(0.0)) (:54).  relin=(evk_ntt, dbc): every power
    relinearised where it is formed (result of size 2 instead of 11)."""
    return _sincos(0, ev, pc, x, zero, relin)


def homomorphic_cos(ev, pc, x, zero, relin=None):
    """homo/fhe_decode.h:128-200 (the reference shifts by -3pi/2 here too, :137, and falls off the end
    without a return statement, :200; the value it leaves in `res` is what is returned here)."""
    return _sincos(1, ev, pc, x, zero, relin)


def stack_zeros(zeros, npos, degree, pos0=0):
    """zeros: callable (i, j, which) -> [1, 2, k, n] -> one tensor [npos, degree, 2, 2, k, n] in the reference's
    call order (position i = pos0 .. pos0 + npos - 1, harmonic j = 1..degree, homomorphic_sin's Enc(0) then homomorphic_cos's)."""
    return torch.cat([zeros(i, j, w) for i in range(pos0, pos0 + npos) for j in range(1, degree + 1) for w in ("sin", "cos")]).contiguous()


def approximated_step(ev, pc, amplitude, index, count, order, degree, delta, width, height, zeros, positions=None, relin=None):
    """The homomorphic overload of approximated_step (homo/fhe_decode.h:202-242) for ONE run
    (fhe_approximated_step).  amplitude/index/count: [1, 2, k, n].  zeros: a tensor [npos, degree, 2, 2, k, n]
    (stack_zeros order) or a callable (i, j, which) -> [1, 2, k, n] encryption of zero for position i, harmonic j,
    which in {"sin", "cos"}.  Returns a list of width*height ciphertexts [1, 22, k, n].

    Faithful to the reference's quirk: `offset` is advanced by add_plain(offset, encode(i)) INSIDE
    the harmonic loop (:229), after cos_arg was copied from it.

    The reference walks positions x harmonics serially with one ciphertext per call; in the library only the
    (cheap) offset chain is serial.  All width*height*degree cosine polynomials are evaluated as ONE
    batch, the sine polynomial once per harmonic (its argument b * f_j does not depend on the
    position) -- the same ring operations on the same operands, so the same bits, but launches that
    fill the GPU.

    positions=(p0, p1) evaluates a SHARD of the output positions (fhe_approximated_step_range; the multi-GPU partition of
    the position loop, :224): zeros (tensor form) and the result then hold positions [p0, p1) only, each bit-identical
    to the whole-run call's.

    relin=(evk_ntt, dbc): the relinearised mode -- every power of the Taylor polynomials, the sin x cos product and the
    final product by the amplitude are relinearised, so the 11 x 11 -> 21 product of the reference's evaluation is a 2 x 2
    one and the results have 2 polynomials instead of 22."""
    cc = circuits_of(pc, relin)
    npos = width * height
    p0, p1 = positions if positions is not None else (0, npos)
    if callable(zeros):
        zeros = stack_zeros(zeros, p1 - p0, degree, p0) if degree > 0 else None
    L = _lib.load()
    so = cc.out_size(STEP, degree)
    out = ev.ctx.empty(p1 - p0, size=so)
    nbytes = L.fhe_approximated_step_range_scratch_bytes(cc.h, degree, npos, p0, p1)
    scr = cc.scratch(nbytes)
    _lib.call("fhe_approximated_step_range", cc.h, _ptr(amplitude), _ptr(index), _ptr(count), order, degree, float(delta), width, height, p0, p1,
              _ptr(zeros) if zeros is not None else C.c_void_p(None), _ptr(out), _ptr(scr), nbytes, _stream())
    return [out[i:i + 1] for i in range(p1 - p0)]


def decode_channel(ev, pc, runs, index, acc0, zeros, order, degree, delta, width, height, positions=None, relin=None):
    """One colour channel of the server_decode driver loop (homo/server_decode.cpp:120-137; fhe_decode_channel).
    runs: [pairs, 2, 2, k, n] (elem, count per run); index: [1, 2, k, n] or [2, k, n], UPDATED IN PLACE (index += count
    per run, :137); acc0: [npos, 2, k, n], the channel's Enc(0) accumulators (:126); zeros: [pairs, npos, degree, 2, 2, k, n].
    Returns [npos, S, k, n], S = 22 for degree >= 1 and pairs > 0.

    positions=(p0, p1): a SHARD of the channel's positions (fhe_decode_channel_range); acc0, zeros and the result hold
    positions [p0, p1) only, and `index` is this shard's own copy of the chain (it ends at the same value on every shard)."""
    cc = circuits_of(pc, relin)
    npos = width * height
    p0, p1 = positions if positions is not None else (0, npos)
    pairs = int(runs.shape[0]) if runs is not None else 0
    assert _count(acc0, 2) == p1 - p0 and index.is_contiguous()
    L = _lib.load()
    so = cc.out_size(DECODE, degree) if pairs else 2
    out = ev.ctx.empty(p1 - p0, size=so)
    nbytes = L.fhe_decode_channel_range_scratch_bytes(cc.h, degree, npos, p0, p1, pairs)
    scr = cc.scratch(nbytes)
    null = C.c_void_p(None)
    _lib.call("fhe_decode_channel_range", cc.h, _ptr(runs) if pairs else null, pairs, _ptr(index), _ptr(acc0),
              _ptr(zeros) if (pairs and degree > 0) else null, order, degree, float(delta), width, height, p0, p1, _ptr(out), _ptr(scr), nbytes, _stream())
    return out


# ---- packed images: one ciphertext holds a tile of pixels in its slots (client.BatchEncoder), a filter is rotations of it -------------
def packed_filter_valid_mask(n, tile_w, kw, kh, anchor=None):
    """[n] bool, flat slot order: where packed_filter2d's window stays inside its tile (each of the two rows of n/2 slots holds one
    row-major tile of tile_w x tile_h pixels) -- everywhere else the rotation wrapped around the row and the value is not the filter's"""
    ax, ay = filter_anchor(kw, kh) if anchor is None else anchor
    half = n // 2
    if tile_w <= 0 or half % tile_w:
        raise ValueError("packed tiles: tile_w = %d does not divide the row of %d slots" % (tile_w, half))
    tile_h = half // tile_w
    y, x = np.divmod(np.arange(half), tile_w)
    ok = (x - ax >= 0) & (x + (kw - 1 - ax) < tile_w) & (y - ay >= 0) & (y + (kh - 1 - ay) < tile_h)
    return np.concatenate([ok, ok])


PACKED_FILTER_PLANS = 16      # RotSumPlans packed_filter2d(fused=True) keeps per SpecialGaloisKeys


def packed_filter_taps(n, t, tile_w, weights_int, kw, kh, anchor=None):
    """([Galois element], [weight mod t]) of packed_filter2d's taps with a non-zero weight, row-major over the kernel with x fastest; the
    tap that does not move is element 1"""
    from .keys import galois_element
    ax, ay = filter_anchor(kw, kh) if anchor is None else anchor
    w = [int(v) for v in np.asarray(weights_int).reshape(-1)]
    if len(w) != kw * kh:
        raise ValueError("packed_filter2d: %d weights for a %d x %d kernel" % (len(w), kw, kh))
    if (n // 2) % tile_w:
        raise ValueError("packed_filter2d: tile_w = %d does not divide the row of %d slots" % (tile_w, n // 2))
    elts, ws = [], []
    for p, wp in enumerate(w):
        if wp % t == 0:
            continue
        j, i = divmod(p, kw)
        elts.append(galois_element(n, (j - ay) * tile_w + (i - ax)))
        ws.append(wp % t)
    if not elts:
        raise ValueError("packed_filter2d: every weight is zero modulo t")
    return elts, ws


def packed_filter2d(ev, keys, ct, tile_w, weights_int, kw, kh, anchor=None, fused=False, border=None):
    """2-D filter with public INTEGER weights over packed tiles: ct [..., 2, k, n] holds, in each row of n/2 slots, a row-major tile of
    tile_w x tile_h pixels.  Output = sum over the taps p = (i, j), row-major over the kernel with x fastest, of
        multiply_plain(rotate_rows(ct, (j - ay) tile_w + (i - ax)), [w_p mod t])
    with zero weights skipped: slot (y, x) of the result is sum_j,i w[j][i] pixel[y + j - ay][x + i - ax] modulo t, exactly, wherever the
    window does not leave the tile (packed_filter_valid_mask); fixed point is the caller's choice of integers, clamp-to-edge is the
    client's padding of the tile.  keys: GaloisKeys (rotations they do not hold directly run as hops, Evaluator.rotate_rows).
    fused=True (opt-in): ONE Evaluator.rotate_sum over all taps -- the forward transforms of c_1 once, one accumulation against every
    tap's key, one set of inverse transforms and one rounding (fhe_rotate_sum_sp).  keys must then be SpecialGaloisKeys that hold every
    tap's element directly (no hops: ValueError otherwise); the plan is kept with the keys (`keys.plans`, at most PACKED_FILTER_PLANS of
    them, the oldest dropped first: a sweep over many filters does not pile up device tables).  The same slots modulo t, a budget of at least rotate_sum_budget; the
    ciphertext bits are NOT those of the default path.  Measured faster than the default path in every case tried (box 3x3 and Gauss 5x5
    at the P8192 and P4096 primes, 256 ciphertexts: 3.2-6.3x).
    border="zero" | "clamp" (opt-in; None: the paths above, as they are): ONE Evaluator.rotate_diag_sum with packed_filter_diagonals'
    per-slot weights -- EVERY slot of the tile is the zero-padded / clamp-to-edge filter's value modulo t, the border included
    (fhe_rotate_diag_sum_sp).  keys: SpecialGaloisKeys that hold every element, the plan is kept as fused=True keeps its
    own; a budget of at least rotate_diag_budget(plan.plains)."""
    ctx = ev.ctx
    if border is not None:
        from .evaluator import RotDiagPlan
        plans = getattr(keys, "plans", None)
        ax, ay = filter_anchor(kw, kh) if anchor is None else anchor
        tag = (tuple(ctx.q), "diag", border, int(tile_w), int(kw), int(kh), int(ax), int(ay), tuple(int(v) % ctx.t for v in np.asarray(weights_int).reshape(-1)))
        plan = plans.get(tag) if plans is not None else None
        if plan is None:
            elts, diags = packed_filter_diagonals(ctx.n, ctx.t, tile_w, weights_int, kw, kh, anchor, border)
            plan = RotDiagPlan(ctx, keys, elts, diags)
            if plans is not None:
                while len(plans) >= PACKED_FILTER_PLANS:
                    del plans[next(iter(plans))]
                plans[tag] = plan
        return ev.rotate_diag_sum(ct, plan)
    if fused:
        from .evaluator import RotSumPlan
        elts, ws = packed_filter_taps(ctx.n, ctx.t, tile_w, weights_int, kw, kh, anchor)
        if len(set(elts)) != len(elts):
            raise ValueError("packed_filter2d(fused=True): two taps of this kernel are the same rotation of the tile")
        plans = getattr(keys, "plans", None)                            # one plan per (level, taps), kept with the keys it points into
        tag = (tuple(ctx.q), tuple(elts), tuple(ws))
        plan = plans.get(tag) if plans is not None else None
        if plan is None:
            plan = RotSumPlan(ctx, keys, elts, ws)
            if plans is not None:
                while len(plans) >= PACKED_FILTER_PLANS:                   # the oldest goes first (a dict keeps insertion order)
                    del plans[next(iter(plans))]
                plans[tag] = plan
        return ev.rotate_sum(ct, plan)
    ax, ay = filter_anchor(kw, kh) if anchor is None else anchor
    w = [int(v) for v in np.asarray(weights_int).reshape(-1)]
    if len(w) != kw * kh:
        raise ValueError("packed_filter2d: %d weights for a %d x %d kernel" % (len(w), kw, kh))
    if (ctx.n // 2) % tile_w:
        raise ValueError("packed_filter2d: tile_w = %d does not divide the row of %d slots" % (tile_w, ctx.n // 2))
    acc = None
    for p, wp in enumerate(w):
        if wp % ctx.t == 0:
            continue
        j, i = divmod(p, kw)
        steps = (j - ay) * tile_w + (i - ax)
        rot = ev.rotate_rows(ct, steps, keys) if ev.rotation_plan(steps, keys) else ct
        term = ev.multiply_plain(rot, np.array([wp % ctx.t], dtype=np.uint64))
        acc = term if acc is None else ev.add(acc, term, out=acc)
    if acc is None:
        raise ValueError("packed_filter2d: every weight is zero modulo t")
    return acc


# ---- packed JPEG: 8x8 blocks packed by POSITION (client.pack_blocks), the transform as integer maps across ciphertexts ----------------
# A fixed-point transform of its own: its ciphertexts and decrypted values are NOT those of fhe_dct8x8_quant / dct8x8_quant, which follow
# the reference's FractionalEncoder circuit.  Values carry `scale_bits` fractional bits; client.descale rounds them away after decryption.
def dct8_matrix(bits=8):
    """[8][8] int64: D[u][x] = round-half-away(2^bits c_u / 2 cos((2 x + 1) u pi / 16)) (fhe_dct8_matrix, host only)"""
    D = np.zeros(64, dtype=np.int64)
    _lib.call("fhe_dct8_matrix", int(bits), D.ctypes.data_as(C.c_void_p))
    return D.reshape(8, 8)


class PackedBlockPlan:
    """The integer map Y = post * (L (pre * X) R^T) of one 8x8 block position-packed over 64 ciphertexts, with its fixed-point scale.
    ctx None: the integers alone (model, bound), no device plan."""

    def __init__(self, ctx, L, R, pre, post, scale_bits):
        self.L, self.R = np.asarray(L, dtype=np.int64).reshape(8, 8), np.asarray(R, dtype=np.int64).reshape(8, 8)
        self.pre = None if pre is None else np.asarray(pre, dtype=np.int64).reshape(8, 8)
        self.post = None if post is None else np.asarray(post, dtype=np.int64).reshape(8, 8)
        self.scale_bits = int(scale_bits)
        self.ctx = ctx
        self.plan = None if ctx is None else Block8x8Plan(ctx, self.L, self.R, self.pre, self.post)

    def model(self, x):
        """the exact integer map on [..., 8, 8] values (Python integers: no overflow)"""
        x = np.asarray(x).astype(object)
        if self.pre is not None:
            x = x * self.pre.astype(object)
        y = np.matmul(np.matmul(self.L.astype(object), x), self.R.astype(object).T)
        return y if self.post is None else y * self.post.astype(object)

    def bound(self, input_bound):
        """the exact worst-case |slot value| of any output for inputs of magnitude at most input_bound (a number, or [8][8] per position):
        max over (u, v) of |post[u][v]| sum_x,y |L[u][x]| |R[v][y]| |pre[x][y]| bound[x][y]; the client picks t > 2 * bound"""
        b = np.broadcast_to(np.asarray(input_bound, dtype=object), (8, 8)) * (1 if self.pre is None else np.abs(self.pre).astype(object))
        y = np.matmul(np.matmul(np.abs(self.L).astype(object), b), np.abs(self.R).astype(object).T)
        if self.post is not None:
            y = y * np.abs(self.post).astype(object)
        return int(y.max())


def _quant8(quant):
    q = np.asarray(quant, dtype=np.int64).reshape(-1)
    if q.size != 64 or (q <= 0).any():
        raise ValueError("a quantisation table has 64 positive integers")
    return q.reshape(8, 8)


def packed_dct_plan(ctx, quant=YQT, dct_bits=8, quant_bits=8):
    """forward 8x8 DCT and quantisation: L = R = D(dct_bits), post[u][v] = round(2^quant_bits / Q[u][v]) = (2^(quant_bits + 1) + Q) // (2 Q);
    the slots hold quantised coefficients times 2^(2 dct_bits + quant_bits)"""
    Q = _quant8(quant)
    D = dct8_matrix(dct_bits)
    post = ((1 << (quant_bits + 1)) + Q) // (2 * Q)
    return PackedBlockPlan(ctx, D, D, None, post, 2 * dct_bits + quant_bits)


def packed_idct_plan(ctx, quant=YQT, dct_bits=8):
    """dequantisation (pre = Q: exact) and the inverse 8x8 DCT: L = R = D(dct_bits)^T; the slots hold pixels times 2^(2 dct_bits)"""
    D = dct8_matrix(dct_bits)
    return PackedBlockPlan(ctx, D.T, D.T, _quant8(quant), None, 2 * dct_bits)


def _round_half_away(v):
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def packed_rgb_to_ycc(bits=8):
    """[3][3] int64: the JFIF RGB -> YCbCr matrix in `bits` fractional bits, each entry rounded half away from zero"""
    m = [[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]]
    return np.array([[_round_half_away(v * (1 << bits)) for v in row] for row in m], dtype=np.int64)


def packed_ycc_to_rgb(bits=8):
    """[3][3] int64: the JFIF YCbCr -> RGB matrix in `bits` fractional bits, each entry rounded half away from zero"""
    m = [[1.0, 0.0, 1.402], [1.0, -0.344136, -0.714136], [1.0, 1.772, 0.0]]
    return np.array([[_round_half_away(v * (1 << bits)) for v in row] for row in m], dtype=np.int64)


def packed_jpeg_compress(ev, plan, r, g, b, colour_bits=8):
    """position-packed R, G, B groups ([groups, 64, size, k, n] each, pixel values 0 .. 255 in the slots) -> [3, groups, 64, size, k, n]:
    the colour mix M = packed_rgb_to_ycc(colour_bits) with the level shift as its bias (Y - 128; the +128 of Cb, Cr and the shift cancel),
    then the block plan per channel (`plan`: one PackedBlockPlan, or three for Y, Cb, Cr).  The slots hold quantised coefficients
    times 2^(plan.scale_bits + colour_bits)."""
    planes = torch.stack([r, g, b]).contiguous()
    ev.channel_mix(packed_rgb_to_ycc(colour_bits), planes, bias=[-(128 << colour_bits), 0, 0], out=planes)
    if isinstance(plan, PackedBlockPlan):
        return ev.block8x8_scalar(plan.plan, planes, out=planes)
    for ch, p in enumerate(plan):
        ev.block8x8_scalar(p.plan, planes[ch], out=planes[ch])
    return planes


# ---- packed frames: pixels packed by POSITION (client.pack_frames / pack_tiles), resize and filters as sparse maps across ciphertexts ----
# Ciphertext p of a frame holds pixel p of n independent frames (or tiles of one image) in its slots.  A resize, a strided filter or a
# chroma subsampling is then one Evaluator.plane_map per pass: integer scalar weights, no rotation, no key (include/fhe_hip.h
# "sparse integer maps across position-packed ciphertexts").  Values carry `scale_bits` fractional bits per plan; client.descale rounds
# them away after decryption.
class PackedPlanePlan:
    """The integer map out[o] = sum_p weights[o][p] * in[taps[o][p]] from n_in to n_out position-packed planes, with its fixed-point
    scale.  ctx None: the integers alone (model, bound), no device plan.  order / window: PlaneMapPlan's."""

    def __init__(self, ctx, n_in, taps, weights, scale_bits=0, order=None, window=0):
        self.taps = np.ascontiguousarray(np.asarray(taps, dtype=np.uint32))
        self.weights = np.ascontiguousarray(np.asarray(weights, dtype=np.int64))
        if self.taps.ndim != 2 or self.taps.shape != self.weights.shape:
            raise ValueError("PackedPlanePlan: taps and weights must both be [n_out][T], got %r and %r" % (self.taps.shape, self.weights.shape))
        self.n_in, self.n_out = int(n_in), int(self.taps.shape[0])
        live = self.weights != 0
        if live.any() and int(self.taps[live].max()) >= self.n_in:
            raise ValueError("PackedPlanePlan: a live tap is not below n_in = %d" % self.n_in)
        self.scale_bits = int(scale_bits)
        self.order = None if order is None else np.ascontiguousarray(np.asarray(order, dtype=np.uint32).reshape(-1))
        self.ctx = ctx
        self.plan = None if ctx is None else PlaneMapPlan(ctx, self.n_in, self.taps, self.weights, order=self.order, window=window)

    def model(self, values):
        """the exact integer map on [n_in, ...] values -> [n_out, ...] (Python integers: no overflow)"""
        v = np.asarray(values).astype(object)
        if v.shape[0] != self.n_in:
            raise ValueError("PackedPlanePlan.model: %d planes for a plan of %d" % (v.shape[0], self.n_in))
        out = np.zeros((self.n_out,) + v.shape[1:], dtype=object)
        w = self.weights.astype(object)
        for p in range(self.taps.shape[1]):
            wp = w[:, p].reshape((-1,) + (1,) * (v.ndim - 1))
            out = out + wp * v[np.where(self.weights[:, p] != 0, self.taps[:, p], 0)]
        return out

    def bound(self, input_bound):
        """the exact worst-case |slot value| of any output for inputs of magnitude at most input_bound (a number, or [n_in] per plane):
        max over o of sum_p |weights[o][p]| bound[taps[o][p]]; the client picks t > 2 * bound"""
        b = np.broadcast_to(np.asarray(input_bound, dtype=object), (self.n_in,))
        w = np.abs(self.weights).astype(object)
        tp = np.where(self.weights != 0, self.taps, 0)
        return int((w * b[tp]).sum(axis=1).max())


def _int_axis(src_len, dst_len, kernel, antialias, convention, weight_bits):
    """(taps [dst][T] clamped, integer weights [dst][T] summing to 2^weight_bits) of one axis"""
    bits = int(weight_bits)
    if not 1 <= bits <= 30:
        raise ValueError("packed resize: weight_bits = %r (1 .. 30: the weights are integers w * 2^bits)" % (weight_bits,))
    taps, w = resample_axis_plan(src_len, dst_len, kernel, antialias, convention, bits)
    wi = np.rint(w * float(1 << bits)).astype(np.int64)               # exact: every weight is a multiple of 2^-bits
    assert np.array_equal(wi.astype(np.float64) / float(1 << bits), w) and (wi.sum(axis=1) == (1 << bits)).all()
    return taps.astype(np.int64), wi


def _resize_pair(ctx, tx, wx, ty, wy, src_w, src_h, bits, window):
    """the horizontal and the vertical PackedPlanePlan of a separable map: axis taps tx [dst_w][Tx] into src_w, ty [dst_h][Ty] into src_h"""
    dst_w, dst_h = tx.shape[0], ty.shape[0]
    line = np.arange(src_h, dtype=np.int64)
    th = (line[:, None, None] * src_w + tx[None, :, :]).reshape(src_h * dst_w, -1)
    wh = np.broadcast_to(wx[None, :, :], (src_h,) + wx.shape).reshape(src_h * dst_w, -1)
    col = np.arange(dst_w, dtype=np.int64)
    tv = (ty[:, None, :] * dst_w + col[None, :, None]).reshape(dst_h * dst_w, -1)
    wv = np.broadcast_to(wy[:, None, :], (dst_h, dst_w, wy.shape[1])).reshape(dst_h * dst_w, -1)
    order = (np.arange(dst_h, dtype=np.int64)[None, :] * dst_w + col[:, None]).reshape(-1)       # column-major: a window holds whole columns
    h = PackedPlanePlan(ctx, src_h * src_w, th, wh, bits, window=window)
    v = PackedPlanePlan(ctx, src_h * dst_w, tv, wv, bits, order=order, window=window)
    return h, v


def packed_resize_plans(ctx, src_w, src_h, dst_w, dst_h, kernel="catmull_rom", antialias=False, convention="half_pixel", weight_bits=8, window=0):
    """(horizontal, vertical): the two PackedPlanePlans of a separable resize of position-packed frames, row-major planes
    [src_h * src_w] -> [src_h * dst_w] -> [dst_h * dst_w].  Each axis is resample_axis_plan with weight_bits: its weights are multiples of
    2^-weight_bits that sum to exactly 1, the integer weights are w * 2^weight_bits; each pass carries scale_bits = weight_bits.  The
    vertical plan cuts its groups along columns."""
    tx, wx = _int_axis(src_w, dst_w, kernel, antialias, convention, weight_bits)
    ty, wy = _int_axis(src_h, dst_h, kernel, antialias, convention, weight_bits)
    return _resize_pair(ctx, tx, wx, ty, wy, src_w, src_h, int(weight_bits), window)


def packed_resize(ev, plans, ct):
    """both passes on frames [..., src_h * src_w, size, k, n] -> [..., dst_h * dst_w, size, k, n]; the slots hold pixels times
    2^(plans[0].scale_bits + plans[1].scale_bits)"""
    return ev.plane_map(plans[1].plan, ev.plane_map(plans[0].plan, ct))


def packed_filter_integer(name):
    """the integer form of a named kernel of FILTERS: dict(weights int64 [kh][kw], divisor, anchor, stride) with weights / divisor the
    float kernel"""
    f = FILTERS[name]
    for div in (1, 4, 9, 16, 256):
        w = f["weights"] * div
        if np.allclose(w, np.rint(w), atol=1e-9):
            return dict(weights=np.rint(w).astype(np.int64), divisor=div, anchor=f["anchor"], stride=f["stride"])
    raise ValueError("filter %r has no small integer form" % name)


def packed_tile_filter_plan(ctx, tile_w, tile_h, weights_int, kw, kh, anchor=None, stride=(1, 1), window=0):
    """A kw x kh filter with public INTEGER weights over position-packed tiles of tile_w x tile_h pixels, clamp-to-edge, the tap geometry
    of filter_tap_plan: planes [tile_h * tile_w] -> [dst_h * dst_w], dst = ceil(tile / stride) per axis (.dst_w, .dst_h); scale_bits 0 --
    dividing by the kernel's divisor is the client's."""
    w = np.asarray(weights_int, dtype=np.int64).reshape(-1)
    if w.size != kw * kh:
        raise ValueError("packed_tile_filter_plan: %d weights for a %d x %d kernel" % (w.size, kw, kh))
    taps, dst_w, dst_h = filter_tap_plan(tile_w, tile_h, kw, kh, 1, anchor, stride)
    plan = PackedPlanePlan(ctx, tile_w * tile_h, taps, np.broadcast_to(w[None, :], taps.shape), 0, window=window)
    plan.dst_w, plan.dst_h = dst_w, dst_h
    return plan


def _tile_axis(src_len, dst_len, core, kernel, antialias, convention, weight_bits):
    """one axis of packed_tile_resize_plans: (frame taps [core_out][T], weights [core_out][T], halo, core_out)"""
    if core <= 0 or src_len % core or (core * dst_len) % src_len:
        raise ValueError("tile resize: a core of %d source samples does not cut %d -> %d into equal tiles (core must divide the source, core * dst / src "
                         "must be an integer)" % (core, src_len, dst_len))
    oc = core * dst_len // src_len
    taps, w = _int_axis(src_len, dst_len, kernel, antialias, convention, weight_bits)
    T = taps.shape[1]
    # the taps of an output are first + p, clamped to the edge: where two neighbours differ, the second one is not clamped
    first = np.zeros(dst_len, dtype=np.int64)
    for x in range(dst_len):
        step = np.nonzero(np.diff(taps[x]))[0]
        first[x] = taps[x][0] if T == 1 else (taps[x][step[0] + 1] - (step[0] + 1) if step.size else (taps[x][0] - (T - 1) if taps[x][0] == 0 else taps[x][0]))
    raw = first[:, None] + np.arange(T, dtype=np.int64)[None, :]
    assert np.array_equal(np.clip(raw, 0, src_len - 1), taps)
    live = w != 0
    s0 = (np.arange(dst_len) // oc * core)[:, None]
    reach = np.maximum(np.maximum(s0 - raw, raw - (s0 + core - 1)), 0)
    halo = int(reach[live].max())
    rebased = np.where(live, raw - (s0 - halo), 0).reshape(dst_len // oc, oc, T)
    wt = w.reshape(dst_len // oc, oc, T)
    if not ((rebased == rebased[:1]).all() and (wt == wt[:1]).all()):
        raise ValueError("tile resize: the tiles of a core of %d source samples (%d -> %d) do not share one plan: their taps or weights differ"
                         % (core, src_len, dst_len))
    return rebased[0], wt[0], halo, oc


def packed_tile_resize_plans(src_w, src_h, dst_w, dst_h, core_w, core_h, kernel="catmull_rom", antialias=False, convention="half_pixel", weight_bits=8,
                             ctx=None, window=0):
    """A large image resized as overlapping tiles in the slots (client.pack_tiles): returns (horizontal, vertical, halo, core_out).  The
    whole-image axis plans are cut into tiles of core_w x core_h source pixels; the outputs of a tile's core have their taps rebased to
    the tile frame, the core plus `halo` = (halo_x, halo_y) pixels on every side (the largest reach of any tap; the image border is the
    client's clamp-to-edge padding).  One pair of frame plans serves every tile: ValueError unless every tile's rebased taps and weights
    are identical (core * dst / src must be an integer per axis).  Planes [(core_h + 2 halo_y) * (core_w + 2 halo_x)] ->
    [core_out_h * core_out_w]; core_out = (w, h) of a tile's output, which client.unpack_tiles stitches."""
    tx, wx, hx, ow = _tile_axis(src_w, dst_w, core_w, kernel, antialias, convention, weight_bits)
    ty, wy, hy, oh = _tile_axis(src_h, dst_h, core_h, kernel, antialias, convention, weight_bits)
    h, v = _resize_pair(ctx, tx, wx, ty, wy, core_w + 2 * hx, core_h + 2 * hy, int(weight_bits), window)
    return h, v, (hx, hy), (ow, oh)


# -- modulus switching (Evaluator.mod_switch): how much budget a switch keeps, how far a result can be switched ------------------------------
def mod_switch_budget(ctx, budget_bits, k_out, size=2):
    """Lower bound (bits, float) on the invariant noise budget of a ciphertext of `size` polynomials under a ternary secret after
    mod_switch to k_out primes, from its budget before.  One drop to the base q' adds at most t S / (2 q') to the invariant noise
    ||v|| = 2^(-B-1), S = 1 + n + .. + n^(size-1) (the rounding error of each polynomial, at most 1/2 per coefficient, times the power of
    the secret it multiplies), so
        B_after >= -log2(2^-B + sum over the bases q' = q_0 .. q_(j-1), j = k - 1 .. k_out, of t S / q').
    Pure Python on ctx.n, ctx.t, ctx.q: `ctx` may be any object with those attributes."""
    from fractions import Fraction
    q, k, k_out = [int(x) for x in ctx.q], len(ctx.q), int(k_out)
    if not 1 <= k_out <= k:
        raise ValueError("mod_switch_budget: k_out = %d of %d primes" % (k_out, k))
    S = sum(int(ctx.n) ** j for j in range(int(size)))
    total = Fraction(1, 1 << int(budget_bits)) if float(budget_bits) == int(budget_bits) else Fraction(2.0 ** -float(budget_bits))
    for j in range(k - 1, k_out - 1, -1):
        total += Fraction(int(ctx.t) * S, math.prod(q[:j]))
    return math.log2(total.denominator) - math.log2(total.numerator)


def special_key_switch_budget(ctx, budget_bits, noise_bound=None):
    """Lower bound (bits, float) on the invariant noise budget after ONE key switch with a special prime (Evaluator.relinearize_sp step,
    apply_galois with SpecialGaloisKeys), from the budget before.  `ctx` is the PARENT context: its last prime p is the special prime, the
    ciphertext lives on the first L = k - 1 primes, Q their product.  The switch adds sum_i d_i e_i / p (d_i a residue polynomial below q_i,
    e_i a key's noise polynomial, n terms per coefficient) and the rounding of the division by p (1/2 per coefficient of u_0, and of u_1
    times the ternary secret):
        E = n B sum_(i < L) (q_i - 1) / p + (1 + n) / 2,        B_after >= -log2(2^-B_before + 2 t E / Q).
    B = noise_bound, the largest absolute value of a key's noise sample; None: what KeyGenerator's sampler can return.  Pure Python on
    ctx.n, ctx.t, ctx.q, as mod_switch_budget."""
    from fractions import Fraction
    q, n = [int(x) for x in ctx.q], int(ctx.n)
    if len(q) < 2:
        raise ValueError("special_key_switch_budget: a context of %d prime(s); the last of at least 2 is the special prime" % len(q))
    if noise_bound is None:
        from .keys import _Sampler
        noise_bound = _Sampler.NOISE_MAX
    p, Q = q[-1], math.prod(q[:-1])
    E = Fraction(n * int(noise_bound) * sum(qi - 1 for qi in q[:-1]), p) + Fraction(1 + n, 2)
    total = Fraction(1, 1 << int(budget_bits)) if float(budget_bits) == int(budget_bits) else Fraction(2.0 ** -float(budget_bits))
    total += 2 * int(ctx.t) * E / Q
    return math.log2(total.denominator) - math.log2(total.numerator)


def rotate_sum_budget(ctx, budget_bits, weights, noise_bound=None):
    """Lower bound (bits, float) on the invariant noise budget after ONE Evaluator.rotate_sum (fhe_rotate_sum_sp) with the given integer
    weights, from the budget before.  `ctx` is the PARENT context (its last prime p is the special prime, Q the product of the others).
    With w'_j the centred lift of w_j modulo t and W = sum_j |w'_j|, the phase of the result is
        sum_j w'_j sigma_(g_j)(c_0 + c_1 s)  +  sum_j w'_j sum_i dig_j,i e_j,i / p  +  rho_0 + rho_1 s            (mod Q):
      * the first term scales the input's invariant noise by at most W -- an automorphism permutes coefficients up to sign, and an integer
        scalar commutes with the scaling by t / Q up to multiples of t, so this factor IS the usual scalar-product term: the (Q mod t) m / Q
        part of the input's invariant noise grows with the rest of it and nothing is added beside it;
      * the digits of tap j are below q_i in magnitude and e_j,i is a key's noise polynomial: at most W n B sum_(i < L) (q_i - 1) / p;
      * ONE rounding whatever the number of taps: 1/2 per coefficient of u_0, and of u_1 times the ternary secret: (1 + n) / 2.
        E = W n B sum_(i < L) (q_i - 1) / p + (1 + n) / 2,        B_after >= -log2(W 2^-B_before + 2 t E / Q).
    B = noise_bound, the largest absolute value of a key's noise sample; None: what KeyGenerator's sampler can return.  Pure Python on
    ctx.n, ctx.t, ctx.q, as special_key_switch_budget (which is the case of one tap of weight 1 that is not the identity)."""
    from fractions import Fraction
    q, n, t = [int(x) for x in ctx.q], int(ctx.n), int(ctx.t)
    if len(q) < 2:
        raise ValueError("rotate_sum_budget: a context of %d prime(s); the last of at least 2 is the special prime" % len(q))
    wc = [int(w) % t for w in np.asarray(weights).reshape(-1)]
    if not wc or any(w == 0 for w in wc):
        raise ValueError("rotate_sum_budget: at least one weight, none of them 0 modulo t")
    W = sum(t - w if 2 * w > t else w for w in wc)
    if noise_bound is None:
        from .keys import _Sampler
        noise_bound = _Sampler.NOISE_MAX
    p, Q = q[-1], math.prod(q[:-1])
    E = Fraction(W * n * int(noise_bound) * sum(qi - 1 for qi in q[:-1]), p) + Fraction(1 + n, 2)
    before = Fraction(1, 1 << int(budget_bits)) if float(budget_bits) == int(budget_bits) else Fraction(2.0 ** -float(budget_bits))
    total = W * before + 2 * t * E / Q
    return math.log2(total.denominator) - math.log2(total.numerator)


def packed_filter_diagonals(n, t, tile_w, weights_int, kw, kh, anchor=None, border="zero"):
    """([Galois element], [G][n] slot values modulo t) of a kw x kh filter over packed tiles that is right at the tile border, for
    RotDiagPlan / Evaluator.rotate_diag_sum: tap (i, j) is the rotation by (j - ay) tile_w + (i - ax), and its diagonal holds, per slot
    (y, x) of the tile (both rows of n/2 slots alike),
        border="zero":   w[j][i] where the source (y + j - ay, x + i - ax) lies inside the tile, 0 elsewhere;
        border="clamp":  clamp-to-edge -- a source outside the tile is the nearest pixel inside it, so w[j][i] is added to the diagonal of
                         the tap that reads THAT pixel from (y, x).  With the anchor inside the kernel the clamped offset lies between 0
                         and the tap's own, inside the kernel's own set of rotations: no further key is needed.
    Taps whose diagonal is 0 in every slot are left out; the tap that does not move is element 1."""
    from .keys import galois_element
    if border not in ("zero", "clamp"):
        raise ValueError("packed_filter_diagonals: border %r (zero, clamp)" % (border,))
    ax, ay = filter_anchor(kw, kh) if anchor is None else anchor
    w = [int(v) for v in np.asarray(weights_int).reshape(-1)]
    if len(w) != kw * kh:
        raise ValueError("packed_filter_diagonals: %d weights for a %d x %d kernel" % (len(w), kw, kh))
    half = n // 2
    if tile_w <= 0 or half % tile_w:
        raise ValueError("packed_filter_diagonals: tile_w = %d does not divide the row of %d slots" % (tile_w, half))
    if border == "clamp" and not (0 <= ax < kw and 0 <= ay < kh):
        raise ValueError("packed_filter_diagonals: border=\"clamp\" needs the anchor inside the kernel")
    tile_h = half // tile_w
    y, x = np.divmod(np.arange(half), tile_w)
    diag = {}                                                           # (dy, dx) -> [half] int64 modulo t
    for p, wp in enumerate(w):
        if wp % t == 0:
            continue
        j, i = divmod(p, kw)
        dy, dx = j - ay, i - ax
        sy, sx = y + dy, x + dx
        inside = (sy >= 0) & (sy < tile_h) & (sx >= 0) & (sx < tile_w)
        if border == "zero":
            d = diag.setdefault((dy, dx), np.zeros(half, dtype=np.int64))
            d[inside] = (d[inside] + wp) % t
            continue
        cy, cx = np.clip(sy, 0, tile_h - 1) - y, np.clip(sx, 0, tile_w - 1) - x
        for off in set(zip(cy.tolist(), cx.tolist())):
            sel = (cy == off[0]) & (cx == off[1])
            d = diag.setdefault(off, np.zeros(half, dtype=np.int64))
            d[sel] = (d[sel] + wp) % t
    elts, rows = [], []
    for (dy, dx), d in sorted(diag.items()):
        if not d.any():
            continue
        elts.append(galois_element(n, dy * tile_w + dx))
        rows.append(np.concatenate([d, d]).astype(np.uint64))
    if not elts:
        raise ValueError("packed_filter_diagonals: every weight is zero modulo t")
    if len(set(elts)) != len(elts):
        raise ValueError("packed_filter_diagonals: two taps of this kernel are the same rotation of the tile")
    return elts, np.stack(rows)


def packed_filter_border_model(tile, weights_int, kw, kh, t, anchor=None, border="zero"):
    """plain numpy: the bordered filter of one tile [tile_h][tile_w] of integers, modulo t (what every slot of
    packed_filter2d(border=...) decrypts to)"""
    ax, ay = filter_anchor(kw, kh) if anchor is None else anchor
    tile = np.asarray(tile).astype(object)
    th, tw = tile.shape
    w = np.asarray(weights_int).reshape(kh, kw)
    out = np.zeros((th, tw), dtype=object)
    for yy in range(th):
        for xx in range(tw):
            acc = 0
            for j in range(kh):
                for i in range(kw):
                    sy, sx = yy + j - ay, xx + i - ax
                    if border == "clamp":
                        sy, sx = min(max(sy, 0), th - 1), min(max(sx, 0), tw - 1)
                    elif not (0 <= sy < th and 0 <= sx < tw):
                        continue
                    acc += int(w[j][i]) * int(tile[sy][sx])
            out[yy][xx] = acc % t
    return out


def block_matvec_diagonals(n, t, B):
    """([Galois element], [G][n] slot values modulo t) of the d x d integer matrix B applied to every aligned group of d slots of both rows
    (the diagonal method): out[g d + a] = sum_b B[a][b] x[g d + b].  d divides n/2.  The steps are -(d - 1) .. d - 1, B[a][b] sits on the
    diagonal of step b - a at the slots = a modulo d; a read that would leave its group meets a 0.  All-zero diagonals are left out."""
    from .keys import galois_element
    B = np.asarray(B)
    if B.ndim != 2 or B.shape[0] != B.shape[1] or B.shape[0] < 1:
        raise ValueError("block_matvec_diagonals: a square matrix expected, got shape %r" % (tuple(B.shape),))
    d, half = int(B.shape[0]), n // 2
    if half % d:
        raise ValueError("block_matvec_diagonals: d = %d does not divide the row of %d slots" % (d, half))
    a = np.arange(n) % d                                                # half is a multiple of d: the same in both rows
    elts, rows = [], []
    for s in range(-(d - 1), d):
        row = np.array([int(B[ai][ai + s]) % t if 0 <= ai + s < d else 0 for ai in a], dtype=np.uint64)
        if not row.any():
            continue
        elts.append(galois_element(n, s))
        rows.append(row)
    if not elts:
        raise ValueError("block_matvec_diagonals: the matrix is zero modulo t")
    return elts, np.stack(rows)


def rotate_diag_budget(ctx, budget_bits, plains, noise_bound=None):
    """Lower bound (bits, float) on the invariant noise budget after ONE Evaluator.rotate_diag_sum (fhe_rotate_diag_sum_sp), from the
    budget before: rotate_sum_budget's formula with W = sum_j ||p'_j||_1, the l1 norm of the centred lift of tap j's plaintext
    (RotDiagPlan.plains: COEFFICIENTS modulo t, not slot values).  A negacyclic product with p'_j scales the coefficients of the input's
    invariant noise, and of the key-switch term, by at most that; the one rounding is as it was.  `ctx` is the PARENT context."""
    from fractions import Fraction
    q, n, t = [int(x) for x in ctx.q], int(ctx.n), int(ctx.t)
    if len(q) < 2:
        raise ValueError("rotate_diag_budget: a context of %d prime(s); the last of at least 2 is the special prime" % len(q))
    P = np.asarray(plains)
    if P.ndim != 2 or P.shape[0] < 1:
        raise ValueError("rotate_diag_budget: plaintexts [G][n] expected")
    W = 0
    for row in P:
        c = [int(v) % t for v in row]
        if not any(c):
            raise ValueError("rotate_diag_budget: a plaintext is the zero polynomial")
        W += sum(t - v if 2 * v > t else v for v in c)
    if noise_bound is None:
        from .keys import _Sampler
        noise_bound = _Sampler.NOISE_MAX
    p, Q = q[-1], math.prod(q[:-1])
    E = Fraction(W * n * int(noise_bound) * sum(qi - 1 for qi in q[:-1]), p) + Fraction(1 + n, 2)
    before = Fraction(1, 1 << int(budget_bits)) if float(budget_bits) == int(budget_bits) else Fraction(2.0 ** -float(budget_bits))
    total = W * before + 2 * t * E / Q
    return math.log2(total.denominator) - math.log2(total.numerator)


def bsgs_split(n, steps, diagonals, baby=None):
    """(baby steps, giant steps, [G2][G1][n] slot values) for RotBsgsPlan(steps=True) from the diagonal form out = sum_s d_s (.) rot_s(x)
    (element 3^s rotates both rows of n/2 slots LEFT by s; steps are signed integers, pairwise distinct as rotations).  Step s is split as
    s = baby a + j with 0 <= j < baby and a = floor(s / baby): baby step j, giant step baby a.  Since rot_g(d (.) y) = rot_g(d) (.) rot_g(y),
    diagonal s is pre-rotated by -baby a within each row: d'_(a,j) = rot_(-baby a)(d_s).  Pairs without a diagonal are all zero (absent).
    baby=None: the power of two nearest sqrt(number of steps)."""
    steps = [int(s) for s in steps]
    d = np.asarray(diagonals)
    half = n // 2
    if d.ndim != 2 or d.shape != (len(steps), n) or not steps:
        raise ValueError("bsgs_split: diagonals of shape %r for %d steps of %d slots" % (tuple(d.shape), len(steps), n))
    if len(set(s % half for s in steps)) != len(steps):
        raise ValueError("bsgs_split: two steps are the same rotation of a row of %d slots" % half)
    if baby is None:
        baby = 1 << max(0, int(round(math.log2(math.sqrt(len(steps))))))
    baby = int(baby)
    if baby < 1:
        raise ValueError("bsgs_split: baby = %d" % baby)
    split = [(s // baby, s % baby) for s in steps]                      # Python's floor division: a < 0 for s < 0, j in [0, baby)
    bs = sorted(set(j for _, j in split))
    gs = sorted(set(a for a, _ in split))
    out = np.zeros((len(gs), len(bs), n), dtype=d.dtype)
    for (a, j), row in zip(split, d):
        out[gs.index(a), bs.index(j)] = np.roll(np.asarray(row).reshape(2, half), baby * a, axis=1).reshape(n)
    return bs, [baby * a for a in gs], out


def block_matvec_bsgs(n, t, B, baby=None):
    """bsgs_split of block_matvec_diagonals(n, t, B): (baby steps, giant steps, [G2][G1][n]) of the d x d matrix B on every aligned group of
    d slots, 2 d - 1 diagonals under about 2 sqrt(2 d) keys"""
    from .keys import galois_element
    elts, diags = block_matvec_diagonals(n, t, B)
    d = int(np.asarray(B).shape[0])
    step_of = {galois_element(n, s): s for s in range(-(d - 1), d)}
    return bsgs_split(n, [step_of[g] for g in elts], diags, baby)


def block_dct2d_matrix(bits=8):
    """[64][64] int64: D (x) D for D = dct8_matrix(bits) -- the 2-D 8 x 8 DCT of a block held row-major in 64 consecutive slots:
    out[8 u + v] = sum_(y, x) D[u][y] D[v][x] block[8 y + x], scaled by 2^(2 bits)"""
    D = dct8_matrix(bits)
    return np.kron(D, D).astype(np.int64)


def rotate_bsgs_budget(ctx, budget_bits, plains, baby, giant, noise_bound=None):
    """Lower bound (bits, float) on the invariant noise budget after ONE Evaluator.rotate_bsgs (fhe_rotate_bsgs_sp), from the budget before.
    `ctx` is the PARENT context; plains [G2][G1][n] are RotBsgsPlan.plains (COEFFICIENTS modulo t, all zero = absent); baby / giant the
    Galois elements (only "is it 1" matters).  With W_i = sum_j ||p'_(i,j)||_1, S = sum_(l < L) (q_l - 1) and B the key noise bound, the
    phase of the result is
        sum_i sigma_(h_i)(X_i)  +  sum_i [ sigma_(h_i)(N_i) / p  +  [h_i != 1] (sigma_(h_i)(rho_i s) + N'_i / p) ]  +  rho_0 + rho_1 s     (mod Q)
      * X_i = sum_j p'_(i,j) sigma_(g_j)(c_0 + c_1 s): the input's invariant noise scaled by at most sum_i W_i;
      * N_i, the inner key-switch terms under the plaintext products: at most W_i n B S each;
      * rho_i, the rounding of v(i), times the ternary secret: n / 2 per non-identity giant step;
      * N'_i, one key switch of v(i) (digits below q_l): n B S per non-identity giant step;
      * the final rounding: (1 + n) / 2.
        E = (sum_i W_i + G') n B S / p + G' n / 2 + (1 + n) / 2,   G' = #{i: h_i != 1},      B_after >= -log2(sum_i W_i 2^-B_before + 2 t E / Q).
    With G2 = 1 and h = {1} this is rotate_diag_budget."""
    from fractions import Fraction
    q, n, t = [int(x) for x in ctx.q], int(ctx.n), int(ctx.t)
    if len(q) < 2:
        raise ValueError("rotate_bsgs_budget: a context of %d prime(s); the last of at least 2 is the special prime" % len(q))
    P = np.asarray(plains)
    giant = [int(h) for h in giant]
    if P.ndim != 3 or P.shape[0] != len(giant) or P.shape[1] != len(list(baby)) or P.shape[0] < 1 or P.shape[1] < 1:
        raise ValueError("rotate_bsgs_budget: plaintexts [G2][G1][n] expected, one row per giant and one column per baby step")
    W = 0
    for row in P:
        Wi = 0
        for pl in row:
            Wi += sum(t - v if 2 * v > t else v for v in (int(x) % t for x in pl))
        if not Wi:
            raise ValueError("rotate_bsgs_budget: a giant step has no present pair")
        W += Wi
    Gn = sum(h != 1 for h in giant)
    if noise_bound is None:
        from .keys import _Sampler
        noise_bound = _Sampler.NOISE_MAX
    p, Q = q[-1], math.prod(q[:-1])
    E = Fraction((W + Gn) * n * int(noise_bound) * sum(qi - 1 for qi in q[:-1]), p) + Fraction(Gn * n, 2) + Fraction(1 + n, 2)
    before = Fraction(1, 1 << int(budget_bits)) if float(budget_bits) == int(budget_bits) else Fraction(2.0 ** -float(budget_bits))
    total = W * before + 2 * t * E / Q
    return math.log2(total.denominator) - math.log2(total.numerator)


def mod_switch_primes(ctx, budget_bits, keep_bits, size=2):
    """The smallest k_out whose mod_switch_budget is at least keep_bits; ctx.k (no switch) when not even one drop qualifies."""
    k = len(ctx.q)
    for k_out in range(1, k):
        if mod_switch_budget(ctx, budget_bits, k_out, size) >= keep_bits:
            return k_out
    return k
