"""Host-side mirror of the SEAL 2.3 objects the reference's circuits use, over the C ABI.

Names follow seal::{EncryptionParameters, SEALContext, FractionalEncoder, Evaluator} as used at
homo/server_jpeg.cpp:74-100 and homo/fhe_image.h:196-325.  Ciphertexts are torch int64 tensors on
the HIP device holding u64 bit patterns, shaped [..., size, k, n] (SEAL-logical order); every
Evaluator method works on whole batches (leading dimensions) in one launch.  PyTorch is used for
device memory and streams only -- all arithmetic happens in libfhe_hip.so.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

# Parameter presets
PRESETS = {
    "P4096": dict(n=4096, q=[0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001], t=1 << 14),
    "P8192": dict(n=8192, q=[0x7FFFFFFF380001, 0x7FFFFFFEF00001, 0x3FFFFFFF000001, 0x3FFFFFFEF40001], t=1 << 14),
    "SEAL23_4096": dict(n=4096, q=[0x7FFFFFFF380001, 0x3FFFFFFF000001], t=1 << 14),
    "SEAL23_2048": dict(n=2048, q=[0x3FFFFFFF000001], t=1 << 14),
    "SEAL23_16384": dict(n=16384, q=[0x7FFFFFFF380001, 0x7FFFFFFEF00001, 0x7FFFFFFEAC0001, 0x7FFFFFFE700001, 0x7FFFFFFE600001, 0x7FFFFFFE4C0001,
                                     0x3FFFFFFF000001, 0x3FFFFFFEF40001], t=1 << 14),      # six 55-bit + two 54-bit primes, 438 bits
    "SEAL3_8192": dict(n=8192, q=[0x7FFFFFD8001, 0x7FFFFFC8001, 0xFFFFFFFC001, 0xFFFFFF6C001, 0xFFFFFEBC001], t=1 << 14),
}
YQT = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
       14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
       49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]  # homo/fhe_image.h:99
SEED = 0x5EA12026


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_EMPTY = {}


def _ptr(t):
    """device pointer of a tensor for the C ABI.  An EMPTY tensor has no storage (data_ptr() == 0) while the library refuses null pointers before it
    looks at the count: an empty batch (a rank whose shard of a small image holds no block, a channel without runs) gets the address of a
    one-word placeholder on the same device instead -- the call is then the no-op the C ABI defines for count == 0."""
    if t.numel() == 0:
        key = (t.device.type, t.device.index)
        if key not in _EMPTY:
            _EMPTY[key] = torch.zeros(2, dtype=torch.int64, device=t.device)
        return C.c_void_p(_EMPTY[key].data_ptr())
    return C.c_void_p(t.data_ptr())


def to_device(arr, device="cuda"):
    """numpy uint64 -> device int64 tensor with the same bits."""
    a = np.ascontiguousarray(arr, dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64)).to(device)


def to_host(t):
    """device int64 tensor -> numpy uint64."""
    return t.detach().cpu().contiguous().numpy().view(np.uint64)


class SEALContext:
    """EncryptionParameters + SEALContext: poly_modulus_degree n, coeff_modulus q[], plain_modulus t."""

    def __init__(self, n, q, t, device=0, switches=None):
        """switches: {"FHE_DCT_FORCE_U64": "1", ...} -- experiment switches for THIS context (the library reads them
        from the environment once, in fhe_ctx_create; they are set around that call only).  Tests and A/B runs."""
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device: this framework has no CPU path")
        self.n, self.q, self.t, self.k = int(n), [int(x) for x in q], int(t), len(q)
        self.device = torch.device("cuda", device)
        arr = (C.c_uint64 * self.k)(*self.q)
        h = C.c_void_p()
        import os
        saved = {name: os.environ.get(name) for name in (switches or {})}
        try:
            for name, value in (switches or {}).items():
                os.environ[name] = str(value)
            _lib.call("fhe_ctx_create", self.n, arr, self.k, self.t, device, C.byref(h))
        finally:
            for name, value in saved.items():
                if value is None:
                    os.environ.pop(name, None)
                else:
                    os.environ[name] = value
        self.h = h

    @classmethod
    def preset(cls, name, device=0, switches=None):
        p = PRESETS[name]
        return cls(p["n"], p["q"], p["t"], device, switches)

    def level(self, k_out):
        """The context a mod_switch result lives in (fhe_ctx_create_level): this context's n, t, device and switches over its first k_out
        primes.  Created on first use and kept for the life of this context; Decryptor(ctx.level(k_out), sk[:k_out]) decrypts there."""
        k_out = int(k_out)
        levels = self.__dict__.setdefault("_levels", {})
        if k_out not in levels:
            h = C.c_void_p()
            _lib.call("fhe_ctx_create_level", self.h, k_out, C.byref(h))
            child = object.__new__(SEALContext)
            child.n, child.q, child.t, child.k, child.device, child.h = self.n, self.q[:k_out], self.t, k_out, self.device, h
            levels[k_out] = child
        return levels[k_out]

    def __del__(self):
        h = getattr(self, "h", None)
        if h:
            try:
                _lib.load().fhe_ctx_destroy(h)
            except Exception:
                pass
            self.h = None

    def ct_shape(self, *lead, size=2):
        return tuple(lead) + (size, self.k, self.n)

    def empty(self, *lead, size=2):
        return torch.empty(self.ct_shape(*lead, size=size), dtype=torch.int64, device=self.device)

    def random_ct(self, *lead, size=2, seed=SEED, first_index=0):
        """Synthetic ciphertexts: splitmix64(seed ^ linear_index) mod q_i."""
        out = self.empty(*lead, size=size)
        n_polys = out.numel() // (self.k * self.n)
        _lib.call("fhe_fill_random", self.h, _ptr(out), n_polys, seed, first_index, _stream())
        return out

    def digest(self, t, index0=0):
        out = torch.zeros(1, dtype=torch.int64, device=self.device)
        _lib.call("fhe_digest", self.h, _ptr(t), t.numel(), index0, _ptr(out), _stream())
        return int(out.cpu().numpy().view(np.uint64)[0])


    def digest_into(self, t, out_elem, index0=0):
        """asynchronous form: the digest of `t` is written to the one-element int64 device tensor `out_elem`"""
        _lib.call("fhe_digest", self.h, _ptr(t), t.numel(), index0, _ptr(out_elem), _stream())


class FractionalEncoder:
    """seal::FractionalEncoder(t, poly_modulus, 100, 100, 2) (homo/server_jpeg.cpp:100)."""

    def __init__(self, ctx, int_coeffs=100, frac_coeffs=100):
        self.ctx, self.int_coeffs, self.frac_coeffs = ctx, int_coeffs, frac_coeffs

    def encode(self, value):
        out = np.zeros(self.ctx.n, dtype=np.uint64)
        _lib.call("fhe_frac_encode", self.ctx.n, self.ctx.t, float(value), self.int_coeffs, self.frac_coeffs,
                  out.ctypes.data_as(C.c_void_p))
        return out

    def decode(self, plain):
        p = np.ascontiguousarray(plain, dtype=np.uint64)
        return float(_lib.load().fhe_frac_decode(self.ctx.n, self.ctx.t, p.ctypes.data_as(C.c_void_p),
                                                 self.int_coeffs, self.frac_coeffs))


SPARSE_MAX_TERMS = 8       # FHE_SPARSE_MAX_TERMS in include/fhe_hip.h


class PreparedPlain:
    """A Plaintext lifted to the q-base and transformed once (the reference redoes this per call)."""

    def __init__(self, ctx, plain):
        self.ctx = ctx
        p = np.ascontiguousarray(plain, dtype=np.uint64)
        nz = np.flatnonzero(p)
        ln = int(nz[-1]) + 1 if nz.size else 0     # significant coefficient count
        self.buf = torch.empty(2 * ctx.k * ctx.n, dtype=torch.int64, device=ctx.device)
        _lib.call("fhe_plain_prepare", ctx.h, p.ctypes.data_as(C.c_void_p), ln, _ptr(self.buf), _stream())
        # few non-zero coefficients (encode(3) = x+1, encode(0.5) = -x^(n-1), ...): the product is a sum
        # of signed rotations, done without any transform (fhe_multiply_plain_sparse)
        self.plain = p[:ln].copy()
        self.sparse = 0 < int(np.count_nonzero(self.plain)) <= SPARSE_MAX_TERMS and ctx.n <= 8192


class PreparedCt:
    """A multiply() operand in prepared form (Evaluator.prepare_operand); opaque device words."""

    def __init__(self, buf, size, lead):
        self.buf, self.size, self.lead = buf, size, lead

    def shared(self, div=1, first=0):
        return SharedPrepared(self, div, first)

    def gather(self, index):
        """The prepared operands `index` (a sequence of positions in the flattened batch, repeats allowed) as a new
        prepared batch -- a copy of words, no arithmetic.  Layout (include/fhe_hip.h, fhe_multiply_prepare):
        [count][size][k][n] over the coefficient base followed by [count][size][k+1][n] over the auxiliary base."""
        count = 1
        for d in self.lead:
            count *= d
        per = self.buf.numel() // count                       # size * (2k + 1) * n
        k = getattr(self, "_k", None)
        if k is None:
            raise ValueError("gather needs a PreparedCt made by Evaluator.prepare_operand")
        qw = per // (2 * k + 1) * k                           # size * k * n
        bw = per - qw                                         # size * (k + 1) * n
        idx = torch.as_tensor(index, dtype=torch.long, device=self.buf.device)
        m = int(idx.numel())
        buf = torch.empty(m * per, dtype=self.buf.dtype, device=self.buf.device)
        torch.index_select(self.buf[:count * qw].view(count, qw), 0, idx, out=buf[:m * qw].view(m, qw))
        torch.index_select(self.buf[count * qw:].view(count, bw), 0, idx, out=buf[m * qw:].view(m, bw))
        out = PreparedCt(buf, self.size, (m,))
        out._k = self._k
        return out


class SharedPrepared:
    """A prepared operand batch shared between the pairs of one multiply(): pair c takes entry
    (first + c // div) % count (fhe_multiply_prepared_shared); PreparedCt.shared(div, first) makes one.
    Right-hand side of multiply() only."""

    def __init__(self, prep, div, first=0):
        count = 1
        for d in prep.lead:
            count *= d
        self.prep, self.div, self.first, self.count, self.size = prep, int(div), int(first), count, prep.size


class DctPlan:
    def __init__(self, ctx, quant=YQT, int_coeffs=100, frac_coeffs=100):
        self.ctx = ctx
        h = C.c_void_p()
        qv = None
        if quant is not None:
            qv = (C.c_double * 64)(*[float(x) for x in quant])
        _lib.call("fhe_dct_plan_create", ctx.h, qv, int_coeffs, frac_coeffs, _stream(), C.byref(h))
        self.h = h

    def __del__(self):
        h = getattr(self, "h", None)
        if h:
            try:
                _lib.load().fhe_dct_plan_destroy(h)
            except Exception:
                pass
            self.h = None


class IdctPlan:
    """Constants of fhe_idct8x8_dequant: dequantisation by `quant` (None: skipped), the twelve line constants, the 1/8 scale."""

    def __init__(self, ctx, quant=YQT, int_coeffs=100, frac_coeffs=100):
        self.ctx = ctx
        h = C.c_void_p()
        qv = None
        if quant is not None:
            if len(quant) != 64:
                raise ValueError("IdctPlan: a quantisation table has 64 entries, got %d" % len(quant))
            qv = (C.c_double * 64)(*[float(x) for x in quant])
        _lib.call("fhe_idct_plan_create", ctx.h, qv, int_coeffs, frac_coeffs, _stream(), C.byref(h))
        self.h = h

    def __del__(self):
        h = getattr(self, "h", None)
        if h:
            try:
                _lib.load().fhe_idct_plan_destroy(h)
            except Exception:
                pass
            self.h = None


FILTER_MAX_TAPS = 64       # FHE_FILTER_MAX_TAPS in include/fhe_hip.h


class FilterPlan:
    """Constants of fhe_filter2d: a 2-D convolution kernel of public weights ([kh][kw], row-major), each distinct weight encoded
    (FractionalEncoder(int_coeffs, frac_coeffs)), lifted and transformed once.  Positions whose weight encodes to zero are skipped."""

    def __init__(self, ctx, weights, int_coeffs=100, frac_coeffs=100):
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.ndim != 2 or w.size == 0:
            raise ValueError("FilterPlan: weights must be a non-empty 2-D array [kh][kw], got shape %r" % (w.shape,))
        if w.size > FILTER_MAX_TAPS:
            raise ValueError("FilterPlan: %d x %d kernel positions, at most FHE_FILTER_MAX_TAPS = %d" % (w.shape[1], w.shape[0], FILTER_MAX_TAPS))
        if not np.all(np.isfinite(w)):
            raise ValueError("FilterPlan: weights must be finite")
        if not np.any(w != 0.0):
            raise ValueError("FilterPlan: every weight is zero (multiply_plain by the zero plaintext is refused)")
        self.ctx, self.weights = ctx, w
        self.kh, self.kw = int(w.shape[0]), int(w.shape[1])
        h = C.c_void_p()
        _lib.call("fhe_filter_plan_create", ctx.h, w.ctypes.data_as(C.c_void_p), self.kw, self.kh, int_coeffs, frac_coeffs, _stream(), C.byref(h))
        self.h = h
        self.taps = int(_lib.call("fhe_filter_plan_taps", h))      # positions whose weight does not encode to zero

    def __del__(self):
        h = getattr(self, "h", None)
        if h:
            try:
                _lib.load().fhe_filter_plan_destroy(h)
            except Exception:
                pass
            self.h = None


REMAP_MAX_TAPS = 64        # FHE_REMAP_MAX_TAPS in include/fhe_hip.h
REMAP_MAX_WEIGHTS = 4096   # FHE_REMAP_MAX_WEIGHTS
REMAP_SKIP = 0xFFFFFFFF    # FHE_REMAP_SKIP: an unused slot of Evaluator.remap's weight ids


class WeightTable:
    """The plaintext weights Evaluator.remap indexes (fhe_weight_table_create): a 1-D array of public values, each distinct one encoded
    (FractionalEncoder(int_coeffs, frac_coeffs)), lifted and transformed once and kept on the device.  Entries that encode to the
    zero plaintext are remembered as such: their slots are skipped."""

    def __init__(self, ctx, values, int_coeffs=100, frac_coeffs=100):
        v = np.ascontiguousarray(values, dtype=np.float64)
        if v.ndim != 1 or v.size == 0:
            raise ValueError("WeightTable: values must be a non-empty 1-D array, got shape %r" % (v.shape,))
        if not np.all(np.isfinite(v)):
            raise ValueError("WeightTable: values must be finite")
        if np.unique(v[v != 0.0]).size > REMAP_MAX_WEIGHTS:
            raise ValueError("WeightTable: %d distinct values, at most FHE_REMAP_MAX_WEIGHTS = %d (round them: weight_bits)"
                             % (np.unique(v[v != 0.0]).size, REMAP_MAX_WEIGHTS))
        self.ctx, self.values = ctx, v
        h = C.c_void_p()
        _lib.call("fhe_weight_table_create", ctx.h, v.ctypes.data_as(C.c_void_p), int(v.size), int_coeffs, frac_coeffs, _stream(), C.byref(h))
        self.h = h
        self.count = int(_lib.call("fhe_weight_table_count", h))
        self.distinct = int(_lib.call("fhe_weight_table_distinct", h))       # distinct entries that do not encode to zero

    def __del__(self):
        h = getattr(self, "h", None)
        if h:
            try:
                _lib.load().fhe_weight_table_destroy(h)
            except Exception:
                pass
            self.h = None


class Block8x8Plan:
    """Constants of fhe_block8x8_scalar (include/fhe_hip.h "integer linear maps across slot-packed ciphertexts"): integer 8x8 matrices L
    (down the columns) and R (along the rows), optional per-input scalars `pre` and per-output scalars `post` ([8][8] or [64], row-major;
    None = all ones).  Every scalar w must satisfy |w| <= min((t - 1) / 2, 2^31 - 1)."""

    def __init__(self, ctx, L, R, pre=None, post=None):
        def arr(a, name):
            if a is None:
                return None
            a = np.ascontiguousarray(np.asarray(a, dtype=np.int64).reshape(-1))
            if a.size != 64:
                raise ValueError("Block8x8Plan: %s must hold 64 integers, got %d" % (name, a.size))
            return a
        self.ctx = ctx
        self.L, self.R, self.pre, self.post = arr(L, "L"), arr(R, "R"), arr(pre, "pre"), arr(post, "post")
        if self.L is None or self.R is None:
            raise ValueError("Block8x8Plan: L and R are required")
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        h = C.c_void_p()
        _lib.call("fhe_block8x8_plan_create", ctx.h, vp(self.L), vp(self.R), vp(self.pre), vp(self.post), _stream(), C.byref(h))
        self.h = h

    def __del__(self):
        h = getattr(self, "h", None)
        if h:
            try:
                _lib.load().fhe_block8x8_plan_destroy(h)
            except Exception:
                pass
            self.h = None


class PlaneMapPlan:
    """Constants of fhe_plane_map (include/fhe_hip.h "sparse integer maps across position-packed ciphertexts"): output plane o is the sum
    over its slots p of weights[o][p] * plane taps[o][p] of the n_in input planes; taps, weights [n_out][T], T <= 64, zero weights are
    skipped slots, |w| <= min((t - 1) / 2, 2^31 - 1).  order: the permutation of the outputs the groups are cut along (None: index order);
    window: 0 (the library's default: the direct kernel, the cut reported for window 16), or 16, 32, 64 (the windowed kernel with that
    cut).  .groups, .source_reads and .window report the cut."""

    def __init__(self, ctx, n_in, taps, weights, order=None, window=0):
        taps = np.ascontiguousarray(np.asarray(taps, dtype=np.uint32))
        weights = np.ascontiguousarray(np.asarray(weights, dtype=np.int64))
        if taps.ndim != 2 or taps.shape != weights.shape:
            raise ValueError("PlaneMapPlan: taps and weights must both be [n_out][T], got %r and %r" % (taps.shape, weights.shape))
        self.ctx, self.n_in, self.n_out, self.T = ctx, int(n_in), int(taps.shape[0]), int(taps.shape[1])
        self.taps, self.weights = taps, weights
        self.order = None if order is None else np.ascontiguousarray(np.asarray(order, dtype=np.uint32).reshape(-1))
        if self.order is not None and self.order.size != self.n_out:
            raise ValueError("PlaneMapPlan: order holds %d entries for %d outputs" % (self.order.size, self.n_out))
        h = C.c_void_p()
        _lib.call("fhe_plane_map_plan_create", ctx.h, self.n_in, self.n_out, self.T, taps.ctypes.data_as(C.c_void_p), weights.ctypes.data_as(C.c_void_p),
                  None if self.order is None else self.order.ctypes.data_as(C.c_void_p), int(window), _stream(), C.byref(h))
        self.h = h
        g, r, w = C.c_uint32(), C.c_uint64(), C.c_uint32()
        _lib.call("fhe_plane_map_plan_info", h, C.byref(g), C.byref(r), C.byref(w))
        self.groups, self.source_reads, self.window = int(g.value), int(r.value), int(w.value)

    def __del__(self):
        h = getattr(self, "h", None)
        if h:
            try:
                _lib.load().fhe_plane_map_plan_destroy(h)
            except Exception:
                pass
            self.h = None


class _RotPlan:
    """What RotSumPlan, RotDiagPlan and RotBsgsPlan share: the checks on the keys and on a list of Galois elements, the key tensors behind
    the bare pointers the library holds, and the plan handle's life.  _STEM: fhe_<_STEM>_plan_create / _scratch_bytes / _plan_destroy."""

    _STEM = None

    def _open(self, ctx_level, keys):
        from .keys import SpecialGaloisKeys                # keys.py imports this module
        if not isinstance(keys, SpecialGaloisKeys):
            raise ValueError("%s: SpecialGaloisKeys expected (KeyGenerator.generate_special_galois_keys), got %s" % (type(self).__name__, type(keys).__name__))
        self.ctx, self.parent = ctx_level, keys.ctx

    def _elements(self, vals, steps, limit, what=None):
        """the Galois elements of one list, counted; what: "baby" / "giant", or None for the taps of a sum"""
        from .keys import galois_element
        elts = [galois_element(int(self.ctx.n), int(v)) if steps else int(v) for v in vals]
        if not 1 <= len(elts) <= limit:
            raise ValueError("%s: %d %s (1 .. %d)" % (type(self).__name__, len(elts), "taps" if what is None else what + " steps", limit))
        return elts

    def _check_elements(self, elts, what=None, tap=None):
        """every element odd, in range and not repeated; tap(j): the family's own check of tap j, after the element's"""
        who, n = type(self).__name__, int(self.ctx.n)
        word = "" if what is None else what + " "
        for j, g in enumerate(elts):
            if not (g & 1) or not 0 < g < 2 * n:
                raise ValueError("%s: %sGalois element %d must be odd and in [1, 2n = %d)" % (who, word, g, 2 * n))
            if g in elts[:j]:
                raise ValueError("%s: %sGalois element %d is repeated" % (who, word, g))
            if tap is not None:
                tap(j)

    def _key_tensors(self, keys, elts):
        """the key tensor of every element (None for 1), under the checks apply_galois makes before a bare pointer is handed over"""
        who, row = type(self).__name__, []
        for g in elts:
            if g == 1:
                row.append(None)
                continue
            if not keys.has(g):
                raise ValueError("%s: no special Galois key for element %d (have %r); the fused call takes no hops" % (who, g, keys.elements()))
            key = keys.key(g)
            check_special_keys(self.ctx, keys.ctx, key, 1, who)
            row.append(key)
        return row

    @staticmethod
    def _key_pointers(row):
        return (C.c_void_p * len(row))(*[None if k is None else k.data_ptr() for k in row])

    def _create(self, *args):
        h = C.c_void_p()
        torch.cuda.synchronize(self.ctx.device)                              # the keys are complete before the plan's own (null-stream) transforms
        _lib.call("fhe_%s_plan_create" % self._STEM, self.parent.h, *args, C.byref(h))
        self.h = h

    def scratch_bytes(self, count):
        return int(getattr(_lib.load(), "fhe_%s_scratch_bytes" % self._STEM)(self.h, int(count)))

    def __del__(self):
        h = getattr(self, "h", None)
        if h:
            try:
                getattr(_lib.load(), "fhe_%s_plan_destroy" % self._STEM)(h)
            except Exception:
                pass
            self.h = None


class RotSumPlan(_RotPlan):
    """The taps of Evaluator.rotate_sum / rotate_each (fhe_rotsum_plan_create: hoisted special-prime rotations of ONE ciphertext).
    ctx_level: the context the ciphertexts live in, the first k - 1 primes of keys.ctx; keys: SpecialGaloisKeys that hold every element
    directly (no hops); elements_or_steps: Galois elements (odd, pairwise distinct, 1 = the ciphertext itself, needs no key), or with
    steps=True row rotations LEFT by that many slots; weights: integers, non-zero modulo t (None: all 1).  The plan keeps the key tensors
    alive: the library holds their device pointers."""

    MAX_TAPS = 64
    _STEM = "rotsum"

    def __init__(self, ctx_level, special_galois_keys, elements_or_steps, weights=None, steps=False):
        keys = special_galois_keys
        self._open(ctx_level, keys)
        t = int(ctx_level.t)
        elts = self._elements(elements_or_steps, steps, self.MAX_TAPS)
        w = [1] * len(elts) if weights is None else [int(v) for v in np.asarray(weights).reshape(-1)]
        if len(w) != len(elts):
            raise ValueError("RotSumPlan: %d weights for %d taps" % (len(w), len(elts)))

        def weight(j):
            if w[j] % t == 0:
                raise ValueError("RotSumPlan: the weight of tap %d is 0 modulo t" % j)
        self._check_elements(elts, tap=weight)
        self._keys = self._key_tensors(keys, elts)
        self.elements, self.weights = elts, [v % t for v in w]
        e = np.array(elts, dtype=np.uint32)
        wv = np.array(self.weights, dtype=np.uint64)
        self._create(len(elts), e.ctypes.data_as(C.c_void_p), wv.ctypes.data_as(C.c_void_p), self._key_pointers(self._keys))

    def scratch_bytes(self, count, each=False):
        return int(_lib.load().fhe_rotsum_scratch_bytes(self.h, int(count), int(bool(each))))


class RotDiagPlan(_RotPlan):
    """The taps of Evaluator.rotate_diag_sum (fhe_rotdiag_plan_create: a diagonal linear map on the slots of ONE ciphertext under one
    special-prime key switch): out = sum_j d_j (.) rot_j(x) slot by slot.  ctx_level, special_galois_keys, elements_or_steps and steps are
    RotSumPlan's; diagonals: [G][n] slot values modulo t in flat row order (row 0 then row 1), none of them all zero -- they go through
    client.BatchEncoder, and the diagonal multiplies AFTER the rotation.  The plan keeps the key tensors alive: the library holds their
    device pointers."""

    MAX_TAPS = 64
    _STEM = "rotdiag"

    def __init__(self, ctx_level, special_galois_keys, elements_or_steps, diagonals, steps=False):
        from .client import BatchEncoder
        keys = special_galois_keys
        self._open(ctx_level, keys)
        n, t = int(ctx_level.n), int(ctx_level.t)
        elts = self._elements(elements_or_steps, steps, self.MAX_TAPS)
        d = np.asarray(diagonals)
        if d.ndim != 2 or d.shape != (len(elts), n):
            raise ValueError("RotDiagPlan: diagonals of shape %r for %d taps of %d slots" % (tuple(d.shape), len(elts), n))
        d = np.array([[int(v) % t for v in row] for row in d], dtype=np.uint64)

        def diagonal(j):
            if not d[j].any():
                raise ValueError("RotDiagPlan: the diagonal of tap %d is 0 modulo t in every slot" % j)
        self._check_elements(elts, tap=diagonal)
        self._keys = self._key_tensors(keys, elts)
        self.elements = elts
        self.plains = np.ascontiguousarray(BatchEncoder(ctx_level).encode_host(d), dtype=np.uint64)      # [G][n] coefficients modulo t
        e = np.array(elts, dtype=np.uint32)
        self._create(len(elts), e.ctypes.data_as(C.c_void_p), self.plains.ctypes.data_as(C.c_void_p), self._key_pointers(self._keys))


class RotBsgsPlan(_RotPlan):
    """The plan of Evaluator.rotate_bsgs (fhe_rotbsgs_plan_create: a baby-step / giant-step linear map on the slots of ONE ciphertext):
    out = sum_i rot_(h_i)( sum_j d_(i,j) (.) rot_(g_j)(x) ) slot by slot, G1 G2 diagonals under G1 + G2 keys.  ctx_level,
    special_galois_keys and steps are RotSumPlan's; baby / giant: the two lists of Galois elements (or row rotations LEFT with steps=True),
    each odd, pairwise distinct, 1 = no rotation, no key; diagonals: [G2][G1][n] slot values modulo t in flat row order -- they go through
    client.BatchEncoder; a diagonal that is 0 in every slot means the pair is absent.  circuits.bsgs_split makes the three from the
    diagonals of a map.  The plan keeps the key tensors alive: the library holds their device pointers."""

    MAX_STEPS = 64
    _STEM = "rotbsgs"

    def __init__(self, ctx_level, special_galois_keys, baby, giant, diagonals, steps=False):
        from .client import BatchEncoder
        keys = special_galois_keys
        self._open(ctx_level, keys)
        n, t = int(ctx_level.n), int(ctx_level.t)
        b = self._elements(baby, steps, self.MAX_STEPS, "baby")
        self._check_elements(b, "baby")
        g = self._elements(giant, steps, self.MAX_STEPS, "giant")
        self._check_elements(g, "giant")
        d = np.asarray(diagonals)
        if d.ndim != 3 or d.shape != (len(g), len(b), n):
            raise ValueError("RotBsgsPlan: diagonals of shape %r for %d giant and %d baby steps of %d slots" % (tuple(d.shape), len(g), len(b), n))
        if d.dtype == object:                                                # Python integers of any size
            d = np.array([int(v) % t for v in d.reshape(-1)], dtype=np.uint64).reshape(d.shape)
        elif d.dtype.kind in "iu":
            d = (d % np.uint64(t) if d.dtype == np.uint64 else d.astype(np.int64) % np.int64(t)).astype(np.uint64)
        else:
            raise ValueError("RotBsgsPlan: integer diagonals expected, got dtype %s" % d.dtype)
        present = d.any(axis=2)
        for i in range(len(g)):
            if not present[i].any():
                raise ValueError("RotBsgsPlan: giant step %d has no present pair (every diagonal of its row is 0 modulo t)" % i)
        for j in range(len(b)):
            if not present[:, j].any():
                raise ValueError("RotBsgsPlan: baby step %d has no present pair (every diagonal of its column is 0 modulo t)" % j)
        self._keys = [self._key_tensors(keys, b), self._key_tensors(keys, g)]
        self.baby, self.giant = b, g
        enc = BatchEncoder(ctx_level).encode_host(d.reshape(len(g) * len(b), n))
        self.plains = np.ascontiguousarray(np.asarray(enc, dtype=np.uint64).reshape(len(g), len(b), n))      # [G2][G1][n] coefficients modulo t
        eb, eg = np.array(b, dtype=np.uint32), np.array(g, dtype=np.uint32)
        self._create(len(b), eb.ctypes.data_as(C.c_void_p), len(g), eg.ctypes.data_as(C.c_void_p), self.plains.ctypes.data_as(C.c_void_p),
                     self._key_pointers(self._keys[0]), self._key_pointers(self._keys[1]))


def check_evaluation_keys(ctx, evk_ntt, dbc, need, who):
    """The library takes the keys as a bare pointer and reads need * fhe_evk_words(ctx, dbc) words behind it (include/fhe_hip.h): the host
    checks that the tensor it hands over holds them -- a key tensor made for another decomposition bit count (fewer digits), another context or
    fewer powers must be an error here, not a read behind the allocation."""
    if not 1 <= int(dbc) <= 60:
        raise ValueError("%s: decomposition bit count %r (1 .. 60)" % (who, dbc))
    if evk_ntt.dtype != torch.int64 or not evk_ntt.is_contiguous() or evk_ntt.device != ctx.device:
        raise ValueError("%s: evaluation keys must be a contiguous int64 tensor on the context's device" % who)
    words = int(_lib.load().fhe_evk_words(ctx.h, int(dbc)))
    if evk_ntt.numel() < need * words:
        raise ValueError("%s: %d key set(s) at dbc %d take %d words on this context, the tensor holds %d (keys generated with another "
                         "decomposition bit count, for another context, or for fewer powers)" % (who, need, dbc, need * words, evk_ntt.numel()))
    nd = int(_lib.load().fhe_evk_digits(ctx.h, int(dbc)))
    if evk_ntt.dim() >= 5 and tuple(evk_ntt.shape[-5:]) != (ctx.k, nd, 2, ctx.k, ctx.n):
        raise ValueError("%s: evaluation keys of shape %r, this context at dbc %d has [k = %d][digits = %d][2][k][n = %d]"
                         % (who, tuple(evk_ntt.shape), dbc, ctx.k, nd, ctx.n))


def check_special_keys(ctx, parent, key, need, who):
    """The same for the special-prime key switch (fhe_relinearize_sp_poly / fhe_apply_galois_sp): `ctx` is the context the ciphertexts live in,
    `parent` the one the keys were generated in.  ctx must be parent's first k - 1 primes with its n, t and device, and the tensor must hold
    `need` key sets of [k - 1][2][k][n] words -- the library reads fhe_ksk_sp_words(parent) words per set behind a bare pointer."""
    if parent.k < 2:
        raise ValueError("%s: the keys' context has %d prime(s); a special-prime key switch needs at least 2" % (who, parent.k))
    if (parent.n, parent.t, parent.device) != (ctx.n, ctx.t, ctx.device) or list(parent.q[:-1]) != list(ctx.q):
        raise ValueError("%s: special-prime keys of another parent context (n = %d, t = %d, k = %d on %s); the ciphertexts' context must be its "
                         "first k - 1 primes (this one has n = %d, t = %d, k = %d on %s)" % (who, parent.n, parent.t, parent.k, parent.device, ctx.n, ctx.t, ctx.k, ctx.device))
    if not isinstance(key, torch.Tensor) or key.dtype != torch.int64 or not key.is_contiguous() or key.device != ctx.device:
        raise ValueError("%s: special-prime keys must be a contiguous int64 tensor on the context's device" % who)
    shape = (parent.k - 1, 2, parent.k, parent.n)
    if key.dim() < 4 or tuple(key.shape[-4:]) != shape or key.numel() < need * int(_lib.load().fhe_ksk_sp_words(parent.h)):
        raise ValueError("%s: %d special-prime key set(s) of shape [k - 1 = %d][2][k = %d][n = %d] expected, got a tensor of shape %r"
                         % ((who, need) + shape[:1] + shape[2:] + (tuple(key.shape),)))


class Evaluator:
    """seal::Evaluator over batches.  In-place semantics of SEAL are expressed functionally:
    every method returns a new tensor unless `out=` is given (which may alias an input)."""

    def __init__(self, ctx):
        self.ctx = ctx
        self._scratch = None

    # -- helpers ---------------------------------------------------------------------------------
    def _npolys(self, t):
        kn = self.ctx.k * self.ctx.n
        assert t.dtype == torch.int64 and t.is_contiguous() and t.numel() % kn == 0
        return t.numel() // kn

    def _scratch_buf(self, nbytes):
        if self._scratch is None or self._scratch.numel() < nbytes:
            self._scratch = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=self.ctx.device)
        return self._scratch

    def _binary(self, name, a, b, out):
        sa, sb = a.shape[-3], b.shape[-3]
        kn = self.ctx.k * self.ctx.n
        if tuple(a.shape[-2:]) != (self.ctx.k, self.ctx.n) or tuple(b.shape[-2:]) != (self.ctx.k, self.ctx.n) or a.numel() // (sa * kn) != b.numel() // (sb * kn):
            raise ValueError("%s: operands of shapes %r and %r are not the same number of ciphertexts of this context (the library reads both with the first one's count)"
                             % (name, tuple(a.shape), tuple(b.shape)))
        if sa == sb:
            if out is not None and (out.numel() != a.numel() or out.dtype != a.dtype or not out.is_contiguous()):
                raise ValueError("%s: `out` must be a contiguous int64 tensor of %d words, got %r" % (name, a.numel(), tuple(out.shape)))
            out = torch.empty_like(a) if out is None else out
            _lib.call(name, self.ctx.h, _ptr(a), _ptr(b), _ptr(out), self._npolys(a), _stream())
            return out
        # unequal sizes: common prefix through the kernel, tail copied (add) or negated (sub of b's tail)
        lead = a.shape[:-3]
        s, m = max(sa, sb), min(sa, sb)
        res = self.ctx.empty(*lead, size=s)
        pa, pb = a[..., :m, :, :].contiguous(), b[..., :m, :, :].contiguous()
        pre = torch.empty_like(pa)
        _lib.call(name, self.ctx.h, _ptr(pa), _ptr(pb), _ptr(pre), self._npolys(pa), _stream())
        res[..., :m, :, :] = pre
        if sa > sb:
            res[..., m:, :, :] = a[..., m:, :, :]
        else:
            tail = b[..., m:, :, :].contiguous()
            if name == "fhe_sub":
                neg = torch.empty_like(tail)
                _lib.call("fhe_negate", self.ctx.h, _ptr(tail), _ptr(neg), self._npolys(tail), _stream())
                tail = neg
            res[..., m:, :, :] = tail
        return res

    # -- seal::Evaluator surface -------------------------------------------------------------------
    def add(self, a, b, out=None):
        return self._binary("fhe_add", a, b, out)

    def sub(self, a, b, out=None):
        return self._binary("fhe_sub", a, b, out)

    def negate(self, a, out=None):
        out = torch.empty_like(a) if out is None else out
        _lib.call("fhe_negate", self.ctx.h, _ptr(a), _ptr(out), self._npolys(a), _stream())
        return out

    def multiply_plain(self, a, plain, out=None):
        if not isinstance(plain, PreparedPlain):
            plain = PreparedPlain(self.ctx, plain)
        out = torch.empty_like(a) if out is None else out
        if plain.sparse:
            _lib.call("fhe_multiply_plain_sparse", self.ctx.h, _ptr(a), _ptr(out), self._npolys(a),
                      plain.plain.ctypes.data_as(C.c_void_p), len(plain.plain), _stream())
        else:
            _lib.call("fhe_multiply_plain", self.ctx.h, _ptr(a), _ptr(out), self._npolys(a), _ptr(plain.buf), _stream())
        return out

    def _plain_addsub(self, a, plain, sign):
        out = a.clone()
        p = np.ascontiguousarray(plain, dtype=np.uint64)
        nz = np.flatnonzero(p)
        ln = int(nz[-1]) + 1 if nz.size else 0     # significant coefficient count
        size = a.shape[-3]
        stride = size * self.ctx.k * self.ctx.n
        count = out.numel() // stride
        _lib.call("fhe_add_plain", self.ctx.h, _ptr(out), stride, count, p.ctypes.data_as(C.c_void_p), ln, sign, _stream())
        return out

    def add_plain(self, a, plain):
        return self._plain_addsub(a, plain, 1)

    def sub_plain(self, a, plain):
        return self._plain_addsub(a, plain, -1)

    def prepare_operand(self, a):
        """Extend a ciphertext batch to the auxiliary base and transform it once, for several multiply()
        calls with the same operand (fhe_multiply_prepare); multiply() accepts the result on either side."""
        size = a.shape[-3]
        lead = tuple(a.shape[:-3])
        count = 1
        for d in lead:
            count *= d
        words = _lib.load().fhe_multiply_operand_words(self.ctx.h, size, count)
        buf = torch.empty(words, dtype=torch.int64, device=self.ctx.device)
        _lib.call("fhe_multiply_prepare", self.ctx.h, _ptr(a), size, count, _ptr(buf), _stream())
        out = PreparedCt(buf, size, lead)
        out._k = self.ctx.k
        return out

    def multiply(self, a, b):
        if isinstance(b, SharedPrepared):
            pa = a if isinstance(a, PreparedCt) else None
            sa = pa.size if pa else a.shape[-3]
            lead = pa.lead if pa else tuple(a.shape[:-3])
            count = 1
            for d in lead:
                count *= d
            out = self.ctx.empty(*lead, size=sa + b.size - 1)
            nbytes = _lib.load().fhe_multiply_scratch_bytes(self.ctx.h, sa, b.size, count)
            scr = self._scratch_buf(nbytes)
            null = C.c_void_p(None)
            _lib.call("fhe_multiply_prepared_shared", self.ctx.h, null if pa else _ptr(a), _ptr(pa.buf) if pa else null, sa,
                      _ptr(b.prep.buf), b.size, b.count, b.div, b.first, _ptr(out), count, _ptr(scr), nbytes, _stream())
            return out
        pa = a if isinstance(a, PreparedCt) else None
        pb = b if isinstance(b, PreparedCt) else None
        sa = pa.size if pa else a.shape[-3]
        sb = pb.size if pb else b.shape[-3]
        lead = pa.lead if pa else tuple(a.shape[:-3])
        assert (pb.lead if pb else tuple(b.shape[:-3])) == lead
        count = 1
        for d in lead:
            count *= d
        out = self.ctx.empty(*lead, size=sa + sb - 1)
        nbytes = _lib.load().fhe_multiply_scratch_bytes(self.ctx.h, sa, sb, count)
        scr = self._scratch_buf(nbytes)
        if pa is None and pb is None:
            _lib.call("fhe_multiply", self.ctx.h, _ptr(a), sa, _ptr(b), sb, _ptr(out), count, _ptr(scr), nbytes, _stream())
        else:
            null = C.c_void_p(None)
            _lib.call("fhe_multiply_prepared", self.ctx.h, null if pa else _ptr(a), _ptr(pa.buf) if pa else null, sa,
                      null if pb else _ptr(b), _ptr(pb.buf) if pb else null, sb, _ptr(out), count, _ptr(scr), nbytes, _stream())
        return out

    def square(self, a):
        sa = a.shape[-3]
        lead = a.shape[:-3]
        count = 1
        for d in lead:
            count *= d
        out = self.ctx.empty(*lead, size=2 * sa - 1)
        nbytes = _lib.load().fhe_multiply_scratch_bytes(self.ctx.h, sa, sa, count)
        scr = self._scratch_buf(nbytes)
        _lib.call("fhe_square", self.ctx.h, _ptr(a), sa, _ptr(out), count, _ptr(scr), nbytes, _stream())
        return out

    def relinearize(self, a, evk_ntt, dbc):
        """evaluator.relinearize(a, evk): ciphertexts of any size >= 2 down to 2, one key switch per polynomial above the second, the top
        one first (SEAL 2.3).  evk_ntt: KeyGenerator.generate_evaluation_keys(dbc) for size 3, generate_evaluation_keys(dbc, size - 2)
        ([size - 2][k][digits][2][k][n]: keys for s^2 .. s^(size-1)) above."""
        size = a.shape[-3]
        if size == 2:
            return a
        kn = self.ctx.k * self.ctx.n
        have = evk_ntt.shape[0] if evk_ntt.dim() == 6 else 1
        if have < size - 2:
            raise ValueError("relinearize: a ciphertext of %d polynomials needs the keys for s^2 .. s^%d (got %d key set(s))" % (size, size - 1, have))
        check_evaluation_keys(self.ctx, evk_ntt, dbc, size - 2, "relinearize")
        work = a.clone()                                   # the steps above the last one run in place
        count = work.numel() // (size * kn)
        out = torch.empty(tuple(a.shape[:-3]) + (2, self.ctx.k, self.ctx.n), dtype=a.dtype, device=a.device)
        nbytes = _lib.load().fhe_relinearize_n_scratch_bytes(self.ctx.h, size, dbc, count)
        scr = self._scratch_buf(nbytes)
        _lib.call("fhe_relinearize_n", self.ctx.h, _ptr(work), size, size * kn, _ptr(out), 2 * kn, count, _ptr(evk_ntt), dbc, _ptr(scr), nbytes, _stream())
        return out

    def relinearize_sp(self, a, keys, parent):
        """relinearize with special-prime keys (fhe_relinearize_sp_poly): this evaluator's context is parent.level(parent.k - 1), `a` a batch of
        ciphertexts of any size >= 2 over its primes, keys = KeyGenerator(parent).generate_special_evaluation_keys(size - 2)
        ([size - 2][k - 1][2][k][n]: the keys for s^2 .. s^(size-1)).  One key switch per polynomial above the second, the top one first."""
        ctx = self.ctx
        if a.dim() < 3 or tuple(a.shape[-2:]) != (ctx.k, ctx.n) or a.dtype != torch.int64 or a.device != ctx.device:
            raise ValueError("relinearize_sp: ciphertexts [..., size, k, n] = [..., size, %d, %d] of this context only, got %r" % (ctx.k, ctx.n, tuple(a.shape)))
        size = a.shape[-3]
        if size == 2:
            return a
        have = keys.shape[0] if isinstance(keys, torch.Tensor) and keys.dim() == 5 else 1
        if have < size - 2:
            raise ValueError("relinearize_sp: a ciphertext of %d polynomials needs the keys for s^2 .. s^%d (got %d key set(s))" % (size, size - 1, have))
        check_special_keys(ctx, parent, keys, size - 2, "relinearize_sp")
        kn = ctx.k * ctx.n
        work = a.contiguous().clone()                      # the steps above the last one run in place
        count = work.numel() // (size * kn)
        out = torch.empty(tuple(a.shape[:-3]) + (2, ctx.k, ctx.n), dtype=a.dtype, device=a.device)
        nbytes = _lib.load().fhe_key_switch_sp_scratch_bytes(parent.h, count)
        scr = self._scratch_buf(nbytes)
        kw = int(_lib.load().fhe_ksk_sp_words(parent.h))
        flat = keys.reshape(-1)
        for p in range(size - 1, 1, -1):
            last = p == 2
            _lib.call("fhe_relinearize_sp_poly", parent.h, _ptr(work), size * kn, p, _ptr(out if last else work), 2 * kn if last else size * kn, count,
                      _ptr(flat[(p - 2) * kw:(p - 1) * kw]), _ptr(scr), nbytes, _stream())
        return out

    # -- seal::Evaluator::rotate_rows / rotate_columns (include/fhe_hip.h: batched slots and Galois rotations) --------
    def _galois_key(self, keys, g, who):
        """the key tensor for element g, refused when the key set belongs to a context of other shapes (the library would read it with
        THIS context's strides) or does not hold the digits of its own dbc"""
        kc = keys.ctx
        if (kc.n, kc.k, kc.device) != (self.ctx.n, self.ctx.k, self.ctx.device) or list(kc.q) != list(self.ctx.q):
            raise ValueError("%s: Galois keys of another context (n = %d, k = %d on %s; this one has n = %d, k = %d on %s)"
                             % (who, kc.n, kc.k, kc.device, self.ctx.n, self.ctx.k, self.ctx.device))
        key = keys.key(g)
        check_evaluation_keys(self.ctx, key, keys.dbc, 1, who)
        return key

    def apply_galois(self, a, g, keys, out=None):
        """sigma_g on a batch of size-2 ciphertexts followed by the key switch back to s (fhe_apply_galois): keys = GaloisKeys holding g,
        or SpecialGaloisKeys of the parent context whose first k - 1 primes are this context's (fhe_apply_galois_sp: the key switch with
        a special prime).  `out` may be `a` itself (in place) or a contiguous tensor of the same shape that does not overlap it."""
        g = int(g)
        if a.dim() < 3 or a.shape[-3] != 2 or tuple(a.shape[-2:]) != (self.ctx.k, self.ctx.n):
            raise ValueError("apply_galois: ciphertexts of size 2 of this context only (SEAL 2.3 refuses other sizes: relinearize first), got %r" % (tuple(a.shape),))
        if not (g & 1) or not 1 < g < 2 * self.ctx.n:
            raise ValueError("apply_galois: Galois element %d must be odd and in (1, 2n = %d)" % (g, 2 * self.ctx.n))
        from .keys import SpecialGaloisKeys                # keys.py imports this module
        special = isinstance(keys, SpecialGaloisKeys)      # keys.ctx is then the PARENT context, this one its first k - 1 primes
        if special:
            key = keys.key(g)
            check_special_keys(self.ctx, keys.ctx, key, 1, "apply_galois")
        else:
            key = self._galois_key(keys, g, "apply_galois")
        if out is not None and (tuple(out.shape) != tuple(a.shape) or out.dtype != a.dtype or not out.is_contiguous() or out.device != a.device):
            raise ValueError("apply_galois: `out` must be a contiguous int64 tensor of shape %r on the input's device" % (tuple(a.shape),))
        out = torch.empty_like(a) if out is None else out
        ctw = 2 * self.ctx.k * self.ctx.n
        count = self._npolys(a) // 2
        if special:
            nbytes = _lib.load().fhe_key_switch_sp_scratch_bytes(keys.ctx.h, count)
            scr = self._scratch_buf(nbytes)
            _lib.call("fhe_apply_galois_sp", keys.ctx.h, _ptr(a), ctw, _ptr(out), ctw, count, g, _ptr(key), _ptr(scr), nbytes, _stream())
            return out
        nbytes = _lib.load().fhe_apply_galois_scratch_bytes(self.ctx.h, keys.dbc, count)
        scr = self._scratch_buf(nbytes)
        _lib.call("fhe_apply_galois", self.ctx.h, _ptr(a), ctw, _ptr(out), ctw, count, g, _ptr(key), keys.dbc, _ptr(scr), nbytes, _stream())
        return out

    def _rotsum_operand(self, a, plan, who, kind=None):
        kind = RotSumPlan if kind is None else kind
        if not isinstance(plan, kind):
            raise ValueError("%s: a %s expected, got %s" % (who, kind.__name__, type(plan).__name__))
        c = plan.ctx
        if (c.n, c.k, c.t, c.device) != (self.ctx.n, self.ctx.k, self.ctx.t, self.ctx.device) or list(c.q) != list(self.ctx.q):
            raise ValueError("%s: the plan was made for another context" % who)
        if a.dim() < 3 or a.shape[-3] != 2 or tuple(a.shape[-2:]) != (self.ctx.k, self.ctx.n):
            raise ValueError("%s: ciphertexts of size 2 of this context only, got %r" % (who, tuple(a.shape)))
        return self._npolys(a) // 2

    def _rotate_fused(self, a, plan, who, kind, entry, out):
        """rotate_sum, rotate_diag_sum and rotate_bsgs: one ciphertext batch in, one out (possibly in place), under one plan"""
        count = self._rotsum_operand(a, plan, who, kind)
        if out is not None and (tuple(out.shape) != tuple(a.shape) or out.dtype != a.dtype or not out.is_contiguous() or out.device != a.device):
            raise ValueError("%s: `out` must be a contiguous int64 tensor of shape %r on the input's device" % (who, tuple(a.shape)))
        out = torch.empty_like(a) if out is None else out
        ctw = 2 * self.ctx.k * self.ctx.n
        nbytes = plan.scratch_bytes(count)
        scr = self._scratch_buf(nbytes)
        _lib.call(entry, plan.h, _ptr(a), ctw, _ptr(out), ctw, count, _ptr(scr), nbytes, _stream())
        return out

    def rotate_sum(self, a, plan, out=None):
        """sum over the plan's taps of w_j * sigma_(g_j)(a), key-switched back to s ONCE (fhe_rotate_sum_sp): one set of forward transforms,
        one accumulation over all taps, one set of inverse transforms and one rounding, whatever the number of taps.  Decrypts to what
        the composition of apply_galois, multiply_plain by the constant w_j and add decrypts to; the ciphertext bits are its own.
        `out` may be `a` itself (in place) or a contiguous tensor of the same shape that does not overlap it."""
        return self._rotate_fused(a, plan, "rotate_sum", RotSumPlan, "fhe_rotate_sum_sp", out)

    def rotate_diag_sum(self, a, plan, out=None):
        """sum over the plan's taps of d_j (.) rot_j(a) slot by slot, key-switched back to s ONCE (fhe_rotate_diag_sum_sp): rotate_sum with
        a vector of slot values per tap where it has one integer -- the diagonal method for a matrix applied to the slot vector, a filter
        that is right at the tile border, a masked move of slots.  Decrypts to what the composition of apply_galois, multiply_plain by the
        encoded diagonal and add decrypts to; the ciphertext bits are its own.  `out` as for rotate_sum."""
        return self._rotate_fused(a, plan, "rotate_diag_sum", RotDiagPlan, "fhe_rotate_diag_sum_sp", out)

    def rotate_bsgs(self, a, plan, out=None):
        """sum_i rot_(h_i)( sum_j d_(i,j) (.) rot_(g_j)(a) ) slot by slot (fhe_rotate_bsgs_sp): the baby-step / giant-step form of
        rotate_diag_sum, G1 + G2 keys for G1 G2 diagonals; c_0 is rounded once.  Decrypts to what the composition of rotate_each,
        multiply_plain, add and apply_galois decrypts to; the ciphertext bits are its own.  `out` as for rotate_sum."""
        return self._rotate_fused(a, plan, "rotate_bsgs", RotBsgsPlan, "fhe_rotate_bsgs_sp", out)

    def rotate_each(self, a, plan):
        """[taps] + a.shape: sigma_(g_j)(a) key-switched back to s for every tap of the plan, the forward transforms shared
        (fhe_rotate_each_sp; the plan's weights are not used).  What per-slot plaintext weights and baby-step / giant-step maps need."""
        count = self._rotsum_operand(a, plan, "rotate_each")
        out = torch.empty((len(plan.elements),) + tuple(a.shape), dtype=a.dtype, device=a.device)
        ctw = 2 * self.ctx.k * self.ctx.n
        nbytes = plan.scratch_bytes(count, each=True)
        scr = self._scratch_buf(nbytes)
        _lib.call("fhe_rotate_each_sp", plan.h, _ptr(a), ctw, _ptr(out), ctw, count * ctw, count, _ptr(scr), nbytes, _stream())
        return out

    def rotation_plan(self, steps, keys):
        """the Galois elements rotate_rows(ct, steps, keys) applies, in order: steps are reduced into (-n/4, n/4]; one element if `keys`
        holds 3^steps mod 2n, otherwise the hops 3^(+-2^i) for the set bits i of |steps|, ascending; [] for steps == 0"""
        n = self.ctx.n
        half = n // 2
        s = int(steps) % half
        if s > half // 2:
            s -= half
        if s == 0:
            return []
        g = self._gal_elt(s)
        if keys.has(g):
            return [g]
        sign = 1 if s > 0 else -1
        return [self._gal_elt(sign * (1 << i)) for i in range(abs(s).bit_length()) if (abs(s) >> i) & 1]

    def _gal_elt(self, steps, swap=False):
        g = C.c_uint32()
        _lib.call("fhe_galois_element", self.ctx.n, int(steps), int(swap), C.byref(g))
        return int(g.value)

    def rotate_rows(self, a, steps, keys, out=None):
        """both rows of slots rotated LEFT by `steps` (negative: right): slot (r, j) of the result is slot (r, j + steps mod n/2) of `a`"""
        plan = self.rotation_plan(steps, keys)
        if not plan:                                                   # a copy, under the checks apply_galois makes
            if a.dim() < 3 or a.shape[-3] != 2 or tuple(a.shape[-2:]) != (self.ctx.k, self.ctx.n):
                raise ValueError("rotate_rows: ciphertexts of size 2 of this context only, got %r" % (tuple(a.shape),))
            if out is None:
                return a.clone()
            if tuple(out.shape) != tuple(a.shape) or out.dtype != a.dtype or not out.is_contiguous() or out.device != a.device:
                raise ValueError("rotate_rows: `out` must be a contiguous int64 tensor of shape %r on the input's device" % (tuple(a.shape),))
            if out is not a:
                out.copy_(a)
            return out
        cur = a
        for g in plan:
            cur = out = self.apply_galois(cur, g, keys, out=out)       # the first hop writes `out`, the others run in place on it
        return out

    def rotate_columns(self, a, keys, out=None):
        """the two rows of slots swapped (g = 2n - 1)"""
        return self.apply_galois(a, 2 * self.ctx.n - 1, keys, out=out)

    # -- integer linear maps across slot-packed ciphertexts (include/fhe_hip.h; csrc/packed.hip) ------------------------------------
    def block8x8_scalar(self, plan, blocks, out=None):
        """Y[u][v] = post[u][v] sum_x,y L[u][x] R[v][y] pre[x][y] X[x][y] on groups of 64 ciphertexts, [..., 64, size, k, n] (ciphertext
        8 x + y of a group is X[x][y]), bit for bit the multiply_plain / add composition; one kernel.  `out` may be `blocks` itself."""
        kn = (self.ctx.k, self.ctx.n)
        if not (isinstance(blocks, torch.Tensor) and blocks.dim() >= 4 and tuple(blocks.shape[-2:]) == kn and blocks.shape[-4] == 64 and blocks.dtype == torch.int64
                and blocks.is_contiguous() and blocks.device == self.ctx.device):
            raise ValueError("block8x8_scalar: `blocks` must be a contiguous int64 tensor [..., 64, size, k, n] = [..., 64, size, %d, %d] on the context's "
                             "device, got %r" % (kn + (tuple(getattr(blocks, "shape", ())),)))
        if plan.ctx is not self.ctx:
            raise ValueError("block8x8_scalar: the plan was built for another context")
        if out is not None and (tuple(out.shape) != tuple(blocks.shape) or out.dtype != blocks.dtype or not out.is_contiguous() or out.device != blocks.device):
            raise ValueError("block8x8_scalar: `out` must be a contiguous tensor like `blocks` (%r), got %r" % (tuple(blocks.shape), tuple(out.shape)))
        out = torch.empty_like(blocks) if out is None else out
        size = int(blocks.shape[-3])
        count = blocks.numel() // (64 * size * kn[0] * kn[1])
        _lib.call("fhe_block8x8_scalar", self.ctx.h, plan.h, _ptr(blocks), _ptr(out), size, count, _stream())
        return out

    def channel_mix(self, M, planes, bias=None, out=None):
        """out_i = sum_j M[i][j] planes_j (+ add_plain of [bias_i mod t]) on planar batches: planes [c, ..., size, k, n], M integers [m][c],
        returns [m, ..., size, k, n]; one kernel (fhe_channel_mix).  `out` may be `planes` itself when m == c."""
        kn = (self.ctx.k, self.ctx.n)
        Mx = np.asarray(M, dtype=np.int64)
        if Mx.ndim != 2 or not (1 <= Mx.shape[0] <= 8 and 1 <= Mx.shape[1] <= 8):
            raise ValueError("channel_mix: M must be an integer matrix [m][c] with 1 <= m, c <= 8, got shape %r" % (Mx.shape,))
        m, c = int(Mx.shape[0]), int(Mx.shape[1])
        if not (isinstance(planes, torch.Tensor) and planes.dim() >= 4 and tuple(planes.shape[-2:]) == kn and planes.shape[0] == c and planes.dtype == torch.int64
                and planes.is_contiguous() and planes.device == self.ctx.device):
            raise ValueError("channel_mix: `planes` must be a contiguous int64 tensor [c = %d, ..., size, k, n] on the context's device, got %r"
                             % (c, tuple(getattr(planes, "shape", ()))))
        shape = (m,) + tuple(planes.shape[1:])
        if out is not None and (tuple(out.shape) != shape or out.dtype != planes.dtype or not out.is_contiguous() or out.device != planes.device):
            raise ValueError("channel_mix: `out` must be a contiguous int64 tensor %r on the input's device, got %r" % (shape, tuple(out.shape)))
        bv = None
        if bias is not None:
            bv = np.ascontiguousarray(np.asarray(bias, dtype=np.int64).reshape(-1))
            if bv.size != m:
                raise ValueError("channel_mix: %d biases for %d outputs" % (bv.size, m))
        out = torch.empty(shape, dtype=torch.int64, device=planes.device) if out is None else out
        size = int(planes.shape[-3])
        ctw = size * kn[0] * kn[1]
        count = planes.numel() // (c * ctw)
        Mx = np.ascontiguousarray(Mx)
        _lib.call("fhe_channel_mix", self.ctx.h, Mx.ctypes.data_as(C.c_void_p), None if bv is None else bv.ctypes.data_as(C.c_void_p), c, m,
                  _ptr(planes), ctw, count * ctw, _ptr(out), ctw, count * ctw, size, count, _stream())
        return out

    def plane_map(self, plan, ct, out=None):
        """out[..., o] = sum_p weights[o][p] * ct[..., taps[o][p]] on frames of position-packed ciphertexts: ct [..., n_in, size, k, n] ->
        [..., n_out, size, k, n], bit for bit the multiply_plain / add composition; one kernel (fhe_plane_map).  `out` may not overlap `ct`."""
        kn = (self.ctx.k, self.ctx.n)
        if plan.ctx is not self.ctx:
            raise ValueError("plane_map: the plan was built for another context")
        if not (isinstance(ct, torch.Tensor) and ct.dim() >= 4 and tuple(ct.shape[-2:]) == kn and ct.shape[-4] == plan.n_in and ct.dtype == torch.int64
                and ct.is_contiguous() and ct.device == self.ctx.device):
            raise ValueError("plane_map: `ct` must be a contiguous int64 tensor [..., n_in, size, k, n] = [..., %d, size, %d, %d] on the context's device, got %r"
                             % ((plan.n_in,) + kn + (tuple(getattr(ct, "shape", ())),)))
        shape = tuple(ct.shape[:-4]) + (plan.n_out,) + tuple(ct.shape[-3:])
        if out is not None and (tuple(out.shape) != shape or out.dtype != ct.dtype or not out.is_contiguous() or out.device != ct.device):
            raise ValueError("plane_map: `out` must be a contiguous int64 tensor %r on the input's device, got %r" % (shape, tuple(out.shape)))
        out = torch.empty(shape, dtype=torch.int64, device=ct.device) if out is None else out
        size = int(ct.shape[-3])
        count = ct.numel() // (plan.n_in * size * kn[0] * kn[1])
        _lib.call("fhe_plane_map", self.ctx.h, plan.h, _ptr(ct), _ptr(out), size, count, _stream())
        return out

    def mod_switch(self, ct, k_out, out=None):
        """Modulus switching (fhe_mod_switch): ct [..., size, k, n] -> [..., size, k_out, n], every polynomial scaled and rounded from this
        context's k primes to its first k_out, one dropped prime after the other, last first.  The result belongs to ctx.level(k_out) and
        decrypts there under sk[:k_out] to the same plaintext; circuits.mod_switch_budget bounds the budget it keeps.  `out` may not overlap `ct`."""
        k, n, k_out = self.ctx.k, self.ctx.n, int(k_out)
        if not (isinstance(ct, torch.Tensor) and ct.dim() >= 3 and tuple(ct.shape[-2:]) == (k, n) and ct.dtype == torch.int64 and ct.is_contiguous()
                and ct.device == self.ctx.device):
            raise ValueError("mod_switch: `ct` must be a contiguous int64 tensor [..., size, k, n] = [..., size, %d, %d] on the context's device, got %r"
                             % (k, n, tuple(getattr(ct, "shape", ()))))
        if not 1 <= k_out < k:
            raise ValueError("mod_switch: k_out = %d, a context of %d primes switches to 1 .. %d" % (k_out, k, k - 1))
        shape = tuple(ct.shape[:-2]) + (k_out, n)
        if out is not None and (tuple(out.shape) != shape or out.dtype != ct.dtype or not out.is_contiguous() or out.device != ct.device):
            raise ValueError("mod_switch: `out` must be a contiguous int64 tensor %r on the input's device, got %r" % (shape, tuple(out.shape)))
        out = torch.empty(shape, dtype=torch.int64, device=ct.device) if out is None else out
        _lib.call("fhe_mod_switch", self.ctx.h, k_out, _ptr(ct), _ptr(out), ct.numel() // (k * n), _stream())
        return out

    def expand_seeded(self, c0, a_key, first_index, out=None):
        """Seeded fresh ciphertexts to ordinary ones (fhe_expand_seeded): c0 [..., k, n] (what keys.SymmetricEncryptor made,
        canonical residues) -> [..., 2, k, n] with c0 in polynomial 0 and a = the expansion of (a_key, first_index + i) in polynomial 1, i the
        flat number of the ciphertext in `c0`.  `out` may not overlap `c0`."""
        k, n = self.ctx.k, self.ctx.n
        if not (isinstance(c0, torch.Tensor) and c0.dim() >= 2 and tuple(c0.shape[-2:]) == (k, n) and c0.dtype == torch.int64 and c0.is_contiguous()
                and c0.device == self.ctx.device):
            raise ValueError("expand_seeded: `c0` must be a contiguous int64 tensor [..., k, n] = [..., %d, %d] on the context's device, got %r"
                             % (k, n, tuple(getattr(c0, "shape", ()))))
        a_key = bytes(a_key)
        if len(a_key) != 32:
            raise ValueError("expand_seeded: a_key has 32 bytes")
        shape = tuple(c0.shape[:-2]) + (2, k, n)
        if out is not None and (tuple(out.shape) != shape or out.dtype != c0.dtype or not out.is_contiguous() or out.device != c0.device):
            raise ValueError("expand_seeded: `out` must be a contiguous int64 tensor %r on the input's device, got %r" % (shape, tuple(out.shape)))
        out = torch.empty(shape, dtype=torch.int64, device=c0.device) if out is None else out
        _lib.call("fhe_expand_seeded", self.ctx.h, _ptr(c0), c0.numel() // (k * n), a_key, int(first_index) & ((1 << 64) - 1), _ptr(out), _stream())
        return out

    # -- primitives named by the north star ---------------------------------------------------------
    def cubic_coeffs(self, A, B, C, D):
        """a = 3B - A - 3C + D, b = 2A - 5B + 4C - D, c = C - A of Cubic (homo/fhe_resize.h:150-172) in one
        pass; valid for the base-2 FractionalEncoder (encode(3) = x+1, ...), which the caller checks."""
        size = A.shape[-3]
        count = A.numel() // (size * self.ctx.k * self.ctx.n)
        a, b, c = torch.empty_like(A), torch.empty_like(A), torch.empty_like(A)
        _lib.call("fhe_cubic_coeffs", self.ctx.h, _ptr(A), _ptr(B), _ptr(C), _ptr(D), _ptr(a), _ptr(b), _ptr(c), size, count, _stream())
        return a, b, c

    def cubic_combine(self, a, b, c, B):
        """0.5 (a + b + c) + B of Cubic (homo/fhe_resize.h:181-188); a, b, c of equal size >= size of B."""
        size_abc, size_b = a.shape[-3], B.shape[-3]
        count = a.numel() // (size_abc * self.ctx.k * self.ctx.n)
        out = torch.empty_like(a)
        _lib.call("fhe_cubic_combine", self.ctx.h, _ptr(a), _ptr(b), _ptr(c), size_abc, _ptr(B), size_b, _ptr(out), count, _stream())
        return out

    def ntt_forward(self, a, out=None):
        out = torch.empty_like(a) if out is None else out
        _lib.call("fhe_ntt_forward", self.ctx.h, _ptr(a), _ptr(out), self._npolys(a), _stream())
        return out

    def ntt_inverse(self, a, out=None):
        out = torch.empty_like(a) if out is None else out
        _lib.call("fhe_ntt_inverse", self.ctx.h, _ptr(a), _ptr(out), self._npolys(a), _stream())
        return out

    def dyadic_multiply(self, a, b, out=None):
        out = torch.empty_like(a) if out is None else out
        _lib.call("fhe_dyadic_multiply", self.ctx.h, _ptr(a), _ptr(b), _ptr(out), self._npolys(a), _stream())
        return out

    # -- fused circuits ---------------------------------------------------------------------------
    def dct8x8_quant(self, plan, blocks, out=None):
        """encrypted_dct + quantize_fhe on [n_blocks, 64, 2, k, n] (homo/fhe_image.h:196-305)."""
        assert blocks.shape[-4:] == (64, 2, self.ctx.k, self.ctx.n) and blocks.is_contiguous()
        if out is not None and (out.shape != blocks.shape or out.dtype != blocks.dtype or not out.is_contiguous() or out.device != blocks.device):
            raise ValueError("dct8x8_quant: `out` must be a contiguous tensor like `blocks` (%r), got %r" % (tuple(blocks.shape), tuple(out.shape)))
        out = torch.empty_like(blocks) if out is None else out
        n_blocks = blocks.numel() // (64 * 2 * self.ctx.k * self.ctx.n)
        nbytes = _lib.load().fhe_dct8x8_scratch_bytes(self.ctx.h, n_blocks)
        scr = self._scratch_buf(nbytes)
        _lib.call("fhe_dct8x8_quant", self.ctx.h, plan.h, _ptr(blocks), _ptr(out), n_blocks, _ptr(scr), nbytes, _stream())
        return out

    def rgb_to_ycc(self, r, g, b, int_coeffs=100, frac_coeffs=100):
        """rgb_to_ycc_fhe on [count, 2, k, n] tensors, in place (homo/fhe_image.h:310-325)."""
        if not (r.shape == g.shape == b.shape and tuple(r.shape[-3:]) == (2, self.ctx.k, self.ctx.n) and r.is_contiguous() and g.is_contiguous() and b.is_contiguous()):
            raise ValueError("rgb_to_ycc: three contiguous tensors of one shape [..., 2, k, n], got %r, %r, %r" % (tuple(r.shape), tuple(g.shape), tuple(b.shape)))
        count = r.numel() // (2 * self.ctx.k * self.ctx.n)
        _lib.call("fhe_rgb_to_ycc", self.ctx.h, _ptr(r), _ptr(g), _ptr(b), count, int_coeffs, frac_coeffs, _stream())
        return r, g, b

    def rgb_to_ycc_blocks(self, blocks, int_coeffs=100, frac_coeffs=100):
        """rgb_to_ycc_fhe on the stream layout [n_blocks, 3, 64, 2, k, n] (64 R, 64 G, 64 B per block), in place."""
        assert blocks.shape[-5:] == (3, 64, 2, self.ctx.k, self.ctx.n) and blocks.is_contiguous()
        n_blocks = blocks.numel() // (3 * 64 * 2 * self.ctx.k * self.ctx.n)
        _lib.call("fhe_rgb_to_ycc_blocks", self.ctx.h, _ptr(blocks), n_blocks, int_coeffs, frac_coeffs, _stream())
        return blocks

    def idct8x8_dequant(self, plan, blocks, out=None):
        """dequantisation + 8x8 inverse DCT on [n_blocks, 64, 2, k, n], the inverse of dct8x8_quant (include/fhe_hip.h)."""
        shape = (64, 2, self.ctx.k, self.ctx.n)
        if not (isinstance(blocks, torch.Tensor) and blocks.dim() >= 4 and tuple(blocks.shape[-4:]) == shape and blocks.dtype == torch.int64
                and blocks.is_contiguous() and blocks.device == self.ctx.device):
            raise ValueError("idct8x8_dequant: `blocks` must be a contiguous int64 tensor [..., 64, 2, k, n] = [..., %d, %d, %d, %d] on the "
                             "context's device, got %r" % (shape + (tuple(getattr(blocks, "shape", ())),)))
        if plan.ctx.k != self.ctx.k or plan.ctx.n != self.ctx.n:
            raise ValueError("idct8x8_dequant: the plan was built for another context")
        if out is not None and (out.shape != blocks.shape or out.dtype != blocks.dtype or not out.is_contiguous() or out.device != blocks.device):
            raise ValueError("idct8x8_dequant: `out` must be a contiguous tensor like `blocks` (%r), got %r" % (tuple(blocks.shape), tuple(out.shape)))
        out = torch.empty_like(blocks) if out is None else out
        n_blocks = blocks.numel() // (64 * 2 * self.ctx.k * self.ctx.n)
        nbytes = _lib.load().fhe_idct8x8_scratch_bytes(self.ctx.h, n_blocks)
        scr = self._scratch_buf(nbytes)
        _lib.call("fhe_idct8x8_dequant", self.ctx.h, plan.h, _ptr(blocks), _ptr(out), n_blocks, _ptr(scr), nbytes, _stream())
        return out

    def ycc_to_rgb_blocks(self, blocks, int_coeffs=100, frac_coeffs=100):
        """JFIF YCbCr -> RGB on the stream layout [n_blocks, 3, 64, 2, k, n] (64 Y, 64 Cb, 64 Cr per block), in place: the inverse of
        rgb_to_ycc_blocks."""
        shape = (3, 64, 2, self.ctx.k, self.ctx.n)
        if not (isinstance(blocks, torch.Tensor) and blocks.dim() >= 5 and tuple(blocks.shape[-5:]) == shape and blocks.dtype == torch.int64
                and blocks.is_contiguous() and blocks.device == self.ctx.device):
            raise ValueError("ycc_to_rgb_blocks: `blocks` must be a contiguous int64 tensor [..., 3, 64, 2, k, n] = [..., %d, %d, %d, %d, %d] on "
                             "the context's device, got %r" % (shape + (tuple(getattr(blocks, "shape", ())),)))
        n_blocks = blocks.numel() // (3 * 64 * 2 * self.ctx.k * self.ctx.n)
        _lib.call("fhe_ycc_to_rgb_blocks", self.ctx.h, _ptr(blocks), n_blocks, int_coeffs, frac_coeffs, _stream())
        return blocks

    def _check_src(self, name, owner, what, src):
        """filter2d / remap: `src` is [..., size, k, n] on this context and `owner` (the plan / weight table, `what` in the message)
        belongs to it.  Returns (size, n_src)."""
        kn = (self.ctx.k, self.ctx.n)
        if not (isinstance(src, torch.Tensor) and src.dim() >= 4 and tuple(src.shape[-2:]) == kn and src.dtype == torch.int64 and src.is_contiguous()
                and src.device == self.ctx.device and src.shape[-3] >= 1):
            raise ValueError("%s: `src` must be a contiguous int64 tensor [..., size, k, n] = [..., size, %d, %d] on the context's device, got %r"
                             % ((name,) + kn + (tuple(getattr(src, "shape", ())),)))
        if owner.ctx is not self.ctx:
            raise ValueError("%s: the %s was built for another context" % (name, what))
        size = int(src.shape[-3])
        return size, src.numel() // (size * kn[0] * kn[1])

    def _check_out(self, name, src, out, count, size):
        """filter2d / remap: `out` is [count, size, k, n] beside `src` and does not overlap it; allocated when None"""
        shape = (count, size, self.ctx.k, self.ctx.n)
        if out is None:
            return torch.empty(shape, dtype=torch.int64, device=src.device)
        if not (isinstance(out, torch.Tensor) and tuple(out.shape) == shape and out.dtype == torch.int64 and out.is_contiguous() and out.device == src.device):
            raise ValueError("%s: `out` must be a contiguous int64 tensor %r on the device of `src`, got %r" % (name, shape, tuple(getattr(out, "shape", ()))))
        a0, a1 = src.data_ptr(), src.data_ptr() + src.numel() * 8
        b0, b1 = out.data_ptr(), out.data_ptr() + out.numel() * 8
        if out.numel() and a0 < b1 and b0 < a1:
            raise ValueError("%s: `out` overlaps `src`" % name)
        return out

    def filter2d(self, plan, src, taps, out=None, src_is_ntt=False):
        """2-D convolution with public weights (fhe_filter2d, include/fhe_hip.h): output c = the sum over the kernel positions p of
        multiply_plain(src[taps[c][p]], encode(w[p])), bit for bit the op-by-op composition, with one forward transform per source
        and one inverse transform per output.  src: [n_src, size, k, n] (never written); taps: [count][kw * kh] indices into src
        (circuits.filter_tap_plan); returns [count, size, k, n].  src_is_ntt: src already is ntt_forward of the ciphertexts."""
        size, n_src = self._check_src("filter2d", plan, "plan", src)
        width = plan.kw * plan.kh
        t = np.asarray(taps)
        if t.ndim != 2 or t.shape[1] != width or t.dtype.kind not in "iu":
            raise ValueError("filter2d: `taps` must be an integer array [count][kw * kh = %d], got shape %r dtype %s" % (width, t.shape, t.dtype))
        if t.size and (int(t.min()) < 0 or int(t.max()) >= n_src):
            raise ValueError("filter2d: taps must index the %d source ciphertexts, got values in [%d, %d]" % (n_src, int(t.min()), int(t.max())))
        t = np.ascontiguousarray(t, dtype=np.uint32)
        count = int(t.shape[0])
        out = self._check_out("filter2d", src, out, count, size)
        if count == 0:
            return out
        nbytes = _lib.load().fhe_filter2d_scratch_bytes(self.ctx.h, plan.h, size, n_src, count, int(bool(src_is_ntt)))
        scr = self._scratch_buf(nbytes)
        _lib.call("fhe_filter2d", self.ctx.h, plan.h, _ptr(src), n_src, size, int(bool(src_is_ntt)), t.ctypes.data_as(C.c_void_p), _ptr(out), count,
                  _ptr(scr), nbytes, _stream())
        return out

    def remap(self, table, src, taps, wids, out=None, src_is_ntt=False, out_is_ntt=False):
        """Resampling with public per-output weights (fhe_remap, include/fhe_hip.h): output c = the sum over the slots p with
        wids[c][p] != REMAP_SKIP (and a weight that does not encode to zero) of multiply_plain(src[taps[c][p]], encode(table.values[wids[c][p]])),
        bit for bit the op-by-op composition.  src: [n_src, size, k, n] (never written); taps, wids: integer arrays [count][T]; returns
        [count, size, k, n].  src_is_ntt: src already is ntt_forward of the ciphertexts; out_is_ntt: the result is left as ntt_forward of
        the specified output (a second remap takes it with src_is_ntt)."""
        size, n_src = self._check_src("remap", table, "weight table", src)
        t, w = np.asarray(taps), np.asarray(wids)
        if t.ndim != 2 or w.shape != t.shape or t.dtype.kind not in "iu" or w.dtype.kind not in "iu" or not 1 <= t.shape[1] <= REMAP_MAX_TAPS:
            raise ValueError("remap: `taps` and `wids` must be integer arrays of one shape [count][T], 1 <= T <= %d, got %r %s and %r %s"
                             % (REMAP_MAX_TAPS, t.shape, t.dtype, w.shape, w.dtype))
        live = w != REMAP_SKIP
        if w.size and (int(w.min()) < 0 or (np.any(live) and int(w[live].max()) >= table.count)):
            raise ValueError("remap: weight ids must index the %d entries of the table (or be REMAP_SKIP)" % table.count)
        if np.any(live) and (int(t[live].min()) < 0 or int(t[live].max()) >= n_src):
            raise ValueError("remap: taps must index the %d source ciphertexts, got values in [%d, %d]" % (n_src, int(t[live].min()), int(t[live].max())))
        if t.shape[0] and not np.all(np.any(live, axis=1)):
            raise ValueError("remap: output %d has no live slot" % int(np.flatnonzero(~np.any(live, axis=1))[0]))
        t = np.ascontiguousarray(np.where(live, t, 0), dtype=np.uint32)
        w = np.ascontiguousarray(w, dtype=np.uint32)
        count, width = int(t.shape[0]), int(t.shape[1])
        out = self._check_out("remap", src, out, count, size)
        if count == 0:
            return out
        nbytes = _lib.load().fhe_remap_scratch_bytes(self.ctx.h, table.h, size, n_src, count, int(bool(src_is_ntt)))
        scr = self._scratch_buf(nbytes)
        _lib.call("fhe_remap", self.ctx.h, table.h, _ptr(src), n_src, size, int(bool(src_is_ntt)), t.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p),
                  width, _ptr(out), int(bool(out_is_ntt)), count, _ptr(scr), nbytes, _stream())
        return out

    def resize_plain(self, plan, src, tables=None, out=None, src_is_ntt=False, int_coeffs=100, frac_coeffs=100):
        """A separable resize with public weights: the two remap passes of `plan` (circuits.resize_plan) with the intermediate kept in NTT
        form, so every ciphertext is transformed forward once and back once.  src: the records of the source rows plan["source_rows"]
        names, [rows * src_w * channels, size, k, n]; returns the records of the plan's destination rows.  tables: the passes' WeightTables
        (built from the plan when None; a server that runs many bands builds them once)."""
        if tables is None:
            tables = [WeightTable(self.ctx, p["values"], int_coeffs, frac_coeffs) for p in plan["passes"]]
        first, second = plan["passes"]
        mid = self.remap(tables[0], src.view(-1, *src.shape[-3:]), first["taps"], first["wids"], src_is_ntt=src_is_ntt, out_is_ntt=True)
        return self.remap(tables[1], mid, second["taps"], second["wids"], out=out, src_is_ntt=True)
