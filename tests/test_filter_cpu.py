"""CPU: the 2-D convolution filters -- the oracle composition of their specification decrypts to the float convolution, the
host-only index arithmetic equals an independent model, the library exports the new entry points, and the Python wrappers refuse
bad operands before any launch.  The GPU kernels are compared with the same composition bit for bit in tests/test_gpu_filter.py."""
import ctypes as C
import re
import types

import numpy as np
import pytest

import filter_oracle as fo

SMALL = dict(n=1024, q=[0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001], t=1 << 14)
NEW_SYMBOLS = ("fhe_filter_plan_create", "fhe_filter_plan_destroy", "fhe_filter_plan_taps", "fhe_filter_tap_plan", "fhe_filter_source_rows",
               "fhe_filter2d_scratch_bytes", "fhe_filter2d", "fhe_filter_path")


@pytest.fixture(scope="module")
def small(oracle_mod):
    orc = oracle_mod.Oracle(SMALL["n"], SMALL["q"], SMALL["t"])
    sk, pk = orc.keygen(seed=3)
    img = np.random.default_rng(65).integers(0, 256, size=(5, 6)).astype(np.float64)
    cts = np.stack([orc.encrypt(pk, orc.encode(float(v)), seed=200 + i) for i, v in enumerate(img.reshape(-1))])
    return orc, sk, img, cts


@pytest.mark.parametrize("kernel", ["box3", "gauss3", "gauss5", "box7", "sobel_x", "sharpen", "chroma420"])
def test_oracle_filter_decrypts_to_float_convolution(small, kernel):
    """fresh encryptions of a 6x5 image of 0..255 at n = 1024, three P4096 primes, t = 2^14"""
    orc, sk, img, cts = small
    weights, anchor, stride = fo.KERNELS[kernel]
    taps = fo.tap_plan(6, 5, 1, weights.shape[1], weights.shape[0], anchor, stride)
    want = fo.conv_float(img, weights, anchor, stride).reshape(-1)
    ops = fo.OracleOps(orc)
    worst, budget = 0.0, 1 << 30
    for o in range(len(taps)):
        plain, b = orc.decrypt(sk, ops.output(cts, taps[o], weights))
        worst, budget = max(worst, abs(orc.decode(plain) - want[o])), min(budget, b)
    print("%s: max |error| = %.3g, noise budget %d bits" % (kernel, worst, budget))
    assert worst < 1e-6
    assert budget > 0


def test_specification_skips_zero_weights(small):
    orc, _, _, cts = small
    ops = fo.OracleOps(orc)
    assert ops.is_zero(0.0) and ops.is_zero(-0.0) and not ops.is_zero(1.0 / 9.0)
    w = fo.KERNELS["sobel_x"][0]
    taps = fo.tap_plan(6, 5, 1, 3, 3, (1, 1), (1, 1))
    six = [p for p in range(9) if w.reshape(-1)[p] != 0]
    acc = None
    for p in six:
        term = ops.M(cts[taps[8][p]], float(w.reshape(-1)[p]))
        acc = term if acc is None else ops.A(acc, term)
    assert np.array_equal(ops.output(cts, taps[8], w), acc)


CASES = [  # src_w, src_h, channels, kw, kh, anchor, stride
    (6, 5, 1, 3, 3, (1, 1), (1, 1)), (6, 5, 3, 3, 3, (1, 1), (1, 1)), (7, 5, 3, 2, 2, (0, 0), (2, 2)), (7, 6, 1, 4, 2, (1, 0), (1, 2)),
    (5, 7, 3, 5, 5, (2, 2), (2, 1)), (1, 4, 3, 3, 3, (1, 1), (1, 1)), (1, 1, 1, 3, 3, (1, 1), (1, 1)), (3, 2, 1, 7, 7, (3, 3), (1, 1)),
    (3, 2, 3, 8, 8, (3, 3), (2, 2)), (6, 5, 1, 3, 3, (0, 2), (1, 1)), (9, 8, 1, 2, 2, (1, 1), (2, 2)),
]


@pytest.mark.parametrize("case", CASES)
def test_tap_plan_and_source_rows_equal_the_model(fhe, case):
    """host only: callable without a device"""
    w, h, ch, kw, kh, anchor, stride = case
    dw, dh = fo.dst_size(w, h, stride)
    none, rw, rh = fhe.filter_tap_plan(w, h, kw, kh, channels=ch, anchor=anchor, stride=stride, taps=False)
    assert none is None and (rw, rh) == (dw, dh)
    taps, rw, rh = fhe.filter_tap_plan(w, h, kw, kh, channels=ch, anchor=anchor, stride=stride, src_row0=0)
    want = fo.tap_plan(w, h, ch, kw, kh, anchor, stride)
    assert (rw, rh) == (dw, dh) and taps.dtype == np.uint32 and np.array_equal(taps, want)
    assert taps.shape == (dw * dh * ch, kw * kh) and int(taps.max()) < w * h * ch
    for cut in range(1, dh):
        for rows in ((0, cut), (cut, dh)):
            first, cnt = fhe.filter_source_rows(h, kh, anchor[1], stride[1], *rows)
            assert (first, cnt) == fo.source_rows(h, kh, anchor[1], stride[1], *rows)
            part, _, _ = fhe.filter_tap_plan(w, h, kw, kh, channels=ch, anchor=anchor, stride=stride, rows=rows)      # window starts at `first`
            model = fo.tap_plan(w, h, ch, kw, kh, anchor, stride, rows=rows, src_row0=first)
            assert np.array_equal(part, model)
            assert int(part.min()) >= 0 and int(part.max()) < cnt * w * ch                                          # inside the resident window
            assert np.array_equal(part + first * w * ch, want[rows[0] * dw * ch:rows[1] * dw * ch])
            # the rows reported are exactly the rows touched
            touched = (part // (w * ch)) + first
            assert int(touched.min()) == first and int(touched.max()) == first + cnt - 1


def test_tap_plan_refuses_bad_geometry(fhe):
    L = fhe._lib
    dw, dh = C.c_uint32(), C.c_uint32()
    args = dict(src_w=6, src_h=5, channels=1, kw=3, kh=3, ax=1, ay=1, sx=1, sy=1, row0=0, row1=5, src_row0=0)
    buf = np.zeros((30, 9), dtype=np.uint32)

    def go(**kw):
        a = dict(args, **kw)
        return L.call("fhe_filter_tap_plan", a["src_w"], a["src_h"], a["channels"], a["kw"], a["kh"], a["ax"], a["ay"], a["sx"], a["sy"], a["row0"], a["row1"],
                      a["src_row0"], C.byref(dw), C.byref(dh), buf.ctypes.data_as(C.c_void_p))
    go()
    for bad in (dict(src_w=0), dict(channels=0), dict(kw=0), dict(kw=9, kh=8), dict(ax=3), dict(ay=-1), dict(sx=0), dict(row0=5), dict(row1=6), dict(row0=2, src_row0=2)):
        with pytest.raises(fhe.FheError):
            go(**bad)
    first, cnt = C.c_uint32(), C.c_uint32()
    with pytest.raises(fhe.FheError):
        L.call("fhe_filter_source_rows", 5, 3, 1, 1, 3, 3, C.byref(first), C.byref(cnt))


def test_library_exports_the_filter_entry_points(fhe):
    lib = C.CDLL(fhe.LIB_PATH)
    hdr = open(fhe.HEADER_PATH).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in fhe._lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert "#define FHE_ABI_VERSION 4" in hdr
    m = re.search(r"#define FHE_FILTER_MAX_TAPS (\d+)", hdr)
    assert m and int(m.group(1)) >= 64 and int(m.group(1)) == fhe.FILTER_MAX_TAPS
    for name in ("box3", "gauss3", "gauss5", "sobel_x", "sobel_y", "laplace", "sharpen", "chroma420"):
        assert name in fhe.FILTERS
    c = fhe.FILTERS["chroma420"]
    assert c["weights"].shape == (2, 2) and np.all(c["weights"] == 0.25) and c["stride"] == (2, 2) and c["anchor"] == (0, 0)
    for name in ("box3", "gauss3", "gauss5", "sobel_x", "sobel_y", "laplace", "sharpen", "chroma420"):
        if name in fo.KERNELS:
            assert np.array_equal(fhe.FILTERS[name]["weights"], fo.KERNELS[name][0]) and tuple(fhe.FILTERS[name]["anchor"]) == fo.KERNELS[name][1]


def _fake_ctx(n=64, k=3):
    import torch
    return types.SimpleNamespace(n=n, k=k, device=torch.device("cpu"), h=None)


def test_filter_wrappers_refuse_bad_operands(fhe):
    """everything below is refused in Python, before any call into the library (the context is a stand-in without a handle)"""
    import torch
    ctx = _fake_ctx()
    ev = fhe.Evaluator(ctx)
    plan = types.SimpleNamespace(ctx=ctx, h=None, kw=3, kh=3)
    src = torch.zeros(4, 2, ctx.k, ctx.n, dtype=torch.int64)
    taps = np.zeros((2, 9), dtype=np.uint32)
    for bad in (torch.zeros(4, 2, ctx.k, ctx.n, dtype=torch.int32),                       # dtype
                torch.zeros(4, 2, ctx.k, 2 * ctx.n, dtype=torch.int64),                   # another n
                torch.zeros(4, 2, ctx.k + 1, ctx.n, dtype=torch.int64),                   # another k
                torch.zeros(2, 4, ctx.k, ctx.n, dtype=torch.int64).transpose(0, 1),       # not contiguous
                torch.zeros(2 * ctx.k * ctx.n, dtype=torch.int64),                        # flat
                np.zeros((4, 2, ctx.k, ctx.n), dtype=np.int64)):                          # not a tensor
        with pytest.raises(ValueError):
            ev.filter2d(plan, bad, taps)
    for bad in (np.zeros((2, 8), dtype=np.uint32), np.zeros(18, dtype=np.uint32), np.full((2, 9), 4, dtype=np.uint32), np.full((2, 9), -1, dtype=np.int64),
                np.zeros((2, 9), dtype=np.float64)):
        with pytest.raises(ValueError):
            ev.filter2d(plan, src, bad)
    for bad in (torch.zeros(3, 2, ctx.k, ctx.n, dtype=torch.int64), torch.zeros(2, 2, ctx.k, ctx.n, dtype=torch.int32),
                torch.zeros(2, 3, ctx.k, ctx.n, dtype=torch.int64), torch.zeros(2, 2, ctx.n, ctx.k, dtype=torch.int64).transpose(2, 3),
                src[1:3], src[:2]):                                                       # the last two overlap src
        with pytest.raises(ValueError):
            ev.filter2d(plan, src, taps, out=bad)
    with pytest.raises(ValueError):
        ev.filter2d(types.SimpleNamespace(ctx=_fake_ctx(), h=None, kw=3, kh=3), src, taps)   # a plan of another context
    for bad in (np.zeros((3, 3)), np.zeros((8, 9)) + 1.0, np.ones(9), np.ones((0, 3)), [[1.0, float("nan")]]):
        with pytest.raises(ValueError):
            fhe.FilterPlan(ctx, bad)
