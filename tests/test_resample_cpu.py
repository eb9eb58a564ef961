"""CPU: resampling with public weights -- the host-only axis plans equal an independent model (tests/resample_oracle.py), the oracle
composition of the two-pass specification decrypts to the float64 resample, the library exports the new entry points, and the Python
wrappers refuse bad operands before any launch.  The GPU kernels are compared with the same composition bit for bit in
tests/test_gpu_resample.py."""
import ctypes as C
import re
import types

import numpy as np
import pytest

import resample_oracle as ro

SMALL = dict(n=1024, q=[0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001], t=1 << 14)
NEW_SYMBOLS = ("fhe_weight_table_create", "fhe_weight_table_destroy", "fhe_weight_table_count", "fhe_weight_table_distinct", "fhe_remap_scratch_bytes",
               "fhe_remap", "fhe_remap_path", "fhe_resample_axis_plan")
SIZES = [(1, 1), (1, 5), (7, 7), (128, 64), (64, 128), (48, 31), (5, 64)]
KERNELS = ["triangle", "catmull_rom", "reference_cubic", "lanczos3", "box"]


@pytest.mark.parametrize("weight_bits", [None, 12])
@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("kernel", KERNELS)
def test_axis_plans_equal_the_model(fhe, kernel, antialias, weight_bits):
    """host only: callable without a device.  Taps are equal; weights are equal to within the last bits of a double (the two sides
    evaluate the same expressions, libm's sin included), exactly equal once rounded to 12 fractional bits; every output's weights sum
    to 1."""
    for convention in ("half_pixel", "reference"):
        for src, dst in SIZES:
            if convention == "reference" and dst < 2:
                with pytest.raises(fhe.FheError):
                    fhe.resample_axis_plan(src, dst, kernel, antialias, convention, weight_bits)
                continue
            taps, weights = fhe.resample_axis_plan(src, dst, kernel, antialias, convention, weight_bits)
            mt, mw = ro.axis_plan(src, dst, kernel, antialias, convention, weight_bits)
            T = ro.axis_width(src, dst, kernel, antialias, convention)
            assert taps.dtype == np.uint32 and taps.shape == weights.shape == (dst, T), (convention, src, dst)
            assert np.array_equal(taps, mt), (convention, src, dst)
            assert int(taps.max()) < src
            if weight_bits:
                assert np.array_equal(weights, mw), (convention, src, dst)
                scaled = weights * (1 << weight_bits)
                assert np.array_equal(scaled, np.round(scaled)) and np.all(scaled.sum(axis=1) == float(1 << weight_bits))
            else:
                assert np.max(np.abs(weights - mw)) <= 1e-15, (convention, src, dst)
                assert np.max(np.abs(weights.sum(axis=1) - 1.0)) <= 1e-14


@pytest.mark.parametrize("kernel", KERNELS)
def test_identity_plan_is_one_tap_of_weight_one(fhe, kernel):
    for n in (1, 7):
        for antialias in (False, True):
            taps, weights = fhe.resample_axis_plan(n, n, kernel, antialias)
            assert np.array_equal(taps, np.arange(n).reshape(n, 1)) and np.array_equal(weights, np.ones((n, 1)))


def test_antialias_widens_the_support_and_refuses_more_than_64_taps(fhe):
    assert fhe.resample_axis_plan(128, 64, "catmull_rom", True)[0].shape[1] == 8
    assert fhe.resample_axis_plan(128, 64, "catmull_rom", False)[0].shape[1] == 4
    assert fhe.resample_axis_plan(64, 128, "lanczos3", True)[0].shape[1] == 6            # enlarging: nothing to widen
    assert fhe.resample_axis_plan(48, 31, "lanczos3", True)[0].shape[1] == 10
    assert fhe.resample_axis_plan(128, 64, "box", True)[0].shape[1] == 2
    assert fhe.resample_axis_plan(320, 30, "lanczos3", True)[0].shape[1] == 64           # c = ceil(3 * 320 / 30) = 32
    with pytest.raises(fhe.FheError):
        fhe.resample_axis_plan(330, 30, "lanczos3", True)                                # c = 33: 66 taps
    assert fhe.resample_axis_plan(330, 30, "lanczos3", False)[0].shape[1] == 6


def test_axis_plan_refusals(fhe):
    L = fhe._lib
    T = C.c_uint32()
    taps, w = np.zeros((4, 4), dtype=np.uint32), np.zeros((4, 4))
    tp, wp = taps.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p)
    L.call("fhe_resample_axis_plan", 8, 4, 1, 0, 0, 0, C.byref(T), tp, wp)
    assert T.value == 4
    for args in ((0, 4, 1, 0, 0, 0), (8, 0, 1, 0, 0, 0), (8, 4, 5, 0, 0, 0), (8, 4, -1, 0, 0, 0), (8, 4, 1, 0, 2, 0), (8, 4, 1, 0, 0, 31), (8, 4, 1, 0, 0, -1),
                 (8, 1, 1, 0, 1, 0),                   # the reference's coordinates divide by dst_len - 1
                 (1000, 10, 3, 1, 0, 0)):              # Lanczos-3 stretched over 100 samples: 600 taps
        with pytest.raises(fhe.FheError):
            L.call("fhe_resample_axis_plan", *args, C.byref(T), tp, wp)
    with pytest.raises(fhe.FheError):
        L.call("fhe_resample_axis_plan", 8, 4, 1, 0, 0, 0, C.byref(T), tp, None)          # taps without weights
    with pytest.raises(fhe.FheError):
        L.call("fhe_resample_axis_plan", 8, 4, 1, 0, 0, 0, None, None, None)


@pytest.mark.parametrize("bicubic", [True, False])
def test_reference_convention_agrees_with_resize_sample_plan(fhe, bicubic):
    """taps and offsets of the REFERENCE convention are those of fhe_resize_sample_plan (the ct x ct circuits' index arithmetic)"""
    kernel = "reference_cubic" if bicubic else "triangle"
    for (sw, sh, dw, dh) in ((8, 6, 5, 4), (6, 8, 12, 11), (128, 128, 64, 64), (5, 5, 2, 2), (3, 1, 7, 9)):
        taps, fx, fy = fhe.circuits.resize_sample_plan(sw, sh, dw, dh, bicubic=bicubic)
        tx, wx = fhe.resample_axis_plan(sw, dw, kernel, False, "reference")
        ty, wy = fhe.resample_axis_plan(sh, dh, kernel, False, "reference")
        nt = 4 if bicubic else 2
        assert tx.shape[1] == ty.shape[1] == nt
        for y in range(dh):
            for x in range(dw):
                o = y * dw + x
                if bicubic:
                    want = [int(ty[y][j]) * sw + int(tx[x][i]) for j in range(4) for i in range(4)]
                else:
                    want = [int(ty[y][i >> 1]) * sw + int(tx[x][i & 1]) for i in range(4)]        # p00, p10, p01, p11
                assert list(taps[o]) == want, (x, y)
                for t, w in ((fx[o], wx[x]), (fy[o], wy[y])):
                    if bicubic:
                        model = [(t * t - t) / 2.0, 1.0 - t * t, (t * t + t) / 2.0, 0.0]
                    else:
                        model = [1.0 - t, t]
                    assert np.max(np.abs(np.array(model) - w)) <= 4e-16, (x, y)


# ---- the oracle composition of the specification --------------------------------------------------------------------------------
IMAGES = ("random", "white", "checker")


@pytest.fixture(scope="module")
def small(oracle_mod):
    orc = oracle_mod.Oracle(SMALL["n"], SMALL["q"], SMALL["t"])
    sk, pk = orc.keygen(seed=3)
    w, h = 7, 6
    imgs = {"random": np.random.default_rng(76).integers(0, 256, size=(h, w)).astype(np.float64), "white": np.full((h, w), 255.0),
            "checker": 255.0 * ((np.arange(h)[:, None] + np.arange(w)[None, :]) % 2)}
    cts = {name: np.stack([orc.encrypt(pk, orc.encode(float(v)), seed=300 + i) for i, v in enumerate(img.reshape(-1))]) for name, img in imgs.items()}
    return orc, sk, imgs, cts


CASES = [  # kernel, dst_w, dst_h, antialias, weight_bits
    ("triangle", 10, 9, False, None), ("triangle", 4, 3, False, None), ("triangle", 4, 3, True, None),
    ("catmull_rom", 10, 9, False, None), ("catmull_rom", 4, 3, False, None), ("catmull_rom", 4, 3, True, None),
    ("lanczos3", 10, 9, False, None), ("lanczos3", 4, 3, False, None), ("lanczos3", 4, 3, True, None),
    ("catmull_rom", 10, 9, False, 12), ("lanczos3", 4, 3, True, 12), ("triangle", 5, 4, False, 12),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%dx%d-aa%d-b%s" % c)
def test_oracle_resize_decrypts_to_float_resample(small, case):
    """fresh encryptions of 7x6 images (0..255, all 255, 0/255 checkerboard) at n = 1024, the three P4096 primes, t = 2^14: the two-pass
    specification decrypts to the float64 resample with the same weights.  The bound 1e-9 is the float64 rounding of at most 64 x 64
    terms of magnitude at most 255 with sum |w| <= 2 per axis (the decoder evaluates an exact dyadic rational in double)."""
    orc, sk, imgs, cts = small
    kernel, dw, dh, antialias, bits = case
    px = ro.axis_plan(7, dw, kernel, antialias, "half_pixel", bits)
    py = ro.axis_plan(6, dh, kernel, antialias, "half_pixel", bits)
    ops = ro.OracleOps(orc)
    picks = sorted({(0, 0), (dw - 1, 0), (0, dh - 1), (dw - 1, dh - 1), (dw // 2, dh // 2), (1, dh - 2)})
    worst, budget = 0.0, 1 << 30
    for name in IMAGES:
        want = ro.resample_float(imgs[name], px, py)
        for (x, y) in picks:
            plain, b = orc.decrypt(sk, ro.resize_output(ops, cts[name], 7, 1, px, py, x, y))
            worst, budget = max(worst, abs(orc.decode(plain) - want[y, x])), min(budget, b)
    print("%s 7x6 -> %dx%d antialias=%d weight_bits=%s: max |error| = %.3g, noise budget %d bits" % (kernel, dw, dh, antialias, bits, worst, budget))
    assert worst < 1e-9
    assert budget > 0


def test_specification_skips_unused_slots_and_zero_weights(small):
    orc, _, _, cts = small
    ops = ro.OracleOps(orc)
    src = cts["random"]
    values = [0.5, 0.0, -0.25, 1e-40]
    assert ops.is_zero(0.0) and ops.is_zero(1e-40) and not ops.is_zero(-0.25)
    got = ops.output(src, [3, 9, 4, 5, 6], [0, 1, ro.SKIP, 3, 2], values)
    want = ops.A(ops.M(src[3], 0.5), ops.M(src[6], -0.25))
    assert np.array_equal(got, want)
    assert ops.output(src, [3, 9], [1, ro.SKIP], values) is None


def test_both_pass_orders_decrypt_alike(small):
    orc, sk, imgs, cts = small
    px, py = ro.axis_plan(7, 4, "catmull_rom"), ro.axis_plan(6, 9, "catmull_rom")
    ops = ro.OracleOps(orc)
    a = ro.resize_output(ops, cts["random"], 7, 1, px, py, 2, 5, order="hv")
    b = ro.resize_output(ops, cts["random"], 7, 1, px, py, 2, 5, order="vh")
    assert orc.decode(orc.decrypt(sk, a)[0]) == orc.decode(orc.decrypt(sk, b)[0])


# ---- exports and wrappers ----------------------------------------------------------------------------------------------------------
def test_library_exports_the_resample_entry_points(fhe):
    lib = C.CDLL(fhe.LIB_PATH)
    hdr = open(fhe.HEADER_PATH).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in fhe._lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert "#define FHE_ABI_VERSION 4" in hdr and lib.fhe_abi_version() == 4
    for macro, value in (("FHE_REMAP_MAX_TAPS", fhe.REMAP_MAX_TAPS), ("FHE_REMAP_MAX_WEIGHTS", fhe.REMAP_MAX_WEIGHTS)):
        m = re.search(r"#define %s (\d+)" % macro, hdr)
        assert m and int(m.group(1)) == value, macro
    assert fhe.REMAP_MAX_TAPS == 64 and fhe.REMAP_SKIP == 0xFFFFFFFF == ro.SKIP and re.search(r"#define FHE_REMAP_SKIP 0xffffffffu", hdr)
    for name, value in ro.KERNELS.items():
        assert fhe.RESAMPLE_KERNELS[name] == value
        assert re.search(r"#define FHE_RESAMPLE_%s %d\b" % (name.upper(), value), hdr), name
    assert fhe.RESAMPLE_CONVENTIONS == {"half_pixel": 0, "reference": 1}
    for name in ("WeightTable", "resample_axis_plan", "resize_plan"):
        assert hasattr(fhe, name), name
    assert hasattr(fhe.Evaluator, "remap") and hasattr(fhe.Evaluator, "resize_plain") and hasattr(fhe.server, "server_resize_plain")


def _fake_ctx(n=64, k=3):
    import torch
    return types.SimpleNamespace(n=n, k=k, device=torch.device("cpu"), h=None)


def test_remap_wrappers_refuse_bad_operands(fhe):
    """everything below is refused in Python, before any call into the library (the context is a stand-in without a handle)"""
    import torch
    ctx = _fake_ctx()
    ev = fhe.Evaluator(ctx)
    table = types.SimpleNamespace(ctx=ctx, h=None, count=5)
    src = torch.zeros(4, 2, ctx.k, ctx.n, dtype=torch.int64)
    taps = np.zeros((2, 3), dtype=np.uint32)
    wids = np.zeros((2, 3), dtype=np.uint32)
    for bad in (torch.zeros(4, 2, ctx.k, ctx.n, dtype=torch.int32),                       # dtype
                torch.zeros(4, 2, ctx.k, 2 * ctx.n, dtype=torch.int64),                   # another n
                torch.zeros(4, 2, ctx.k + 1, ctx.n, dtype=torch.int64),                   # another k
                torch.zeros(2, 4, ctx.k, ctx.n, dtype=torch.int64).transpose(0, 1),       # not contiguous
                torch.zeros(2 * ctx.k * ctx.n, dtype=torch.int64),                        # flat
                np.zeros((4, 2, ctx.k, ctx.n), dtype=np.int64)):                          # not a tensor
        with pytest.raises(ValueError):
            ev.remap(table, bad, taps, wids)
    skip_row = np.array([[0, 0, 0], [fhe.REMAP_SKIP] * 3], dtype=np.uint32)
    for bad_t, bad_w in ((np.zeros((2, 4), dtype=np.uint32), wids), (np.zeros(6, dtype=np.uint32), np.zeros(6, dtype=np.uint32)),
                         (np.full((2, 3), 4, dtype=np.uint32), wids), (np.full((2, 3), -1, dtype=np.int64), wids), (np.zeros((2, 3)), wids),
                         (taps, np.full((2, 3), 5, dtype=np.uint32)), (taps, np.full((2, 3), -1, dtype=np.int64)), (taps, np.zeros((2, 3))),
                         (taps, skip_row),                                                # an output without a live slot
                         (np.zeros((2, 65), dtype=np.uint32), np.zeros((2, 65), dtype=np.uint32)), (np.zeros((2, 0), dtype=np.uint32), np.zeros((2, 0), dtype=np.uint32))):
        with pytest.raises(ValueError):
            ev.remap(table, src, bad_t, bad_w)
    for bad in (torch.zeros(3, 2, ctx.k, ctx.n, dtype=torch.int64), torch.zeros(2, 2, ctx.k, ctx.n, dtype=torch.int32),
                torch.zeros(2, 3, ctx.k, ctx.n, dtype=torch.int64), torch.zeros(2, 2, ctx.n, ctx.k, dtype=torch.int64).transpose(2, 3),
                src[1:3], src[:2]):                                                       # the last two overlap src
        with pytest.raises(ValueError):
            ev.remap(table, src, taps, wids, out=bad)
    with pytest.raises(ValueError):
        ev.remap(types.SimpleNamespace(ctx=_fake_ctx(), h=None, count=5), src, taps, wids)   # a table of another context
    for bad in (np.zeros((3, 3)), np.ones(0), [1.0, float("nan")], [float("inf")], np.arange(1, 4098) / 8192.0):
        with pytest.raises(ValueError):
            fhe.WeightTable(ctx, bad)


def test_resize_plan_composes_the_axis_plans(fhe):
    """the 2-D plan is the axis plans laid over the interleaved record order; a shard's window holds exactly the rows it reads; both
    orders describe the same map"""
    sw, sh, dw, dh, ch = 7, 6, 4, 9, 3
    px, py = ro.axis_plan(sw, dw, "catmull_rom"), ro.axis_plan(sh, dh, "catmull_rom")
    img = np.random.default_rng(9).integers(0, 256, size=(sh, sw, ch)).astype(np.float64)
    want = ro.resample_float(img, px, py)

    def run(plan, window):
        data = window.reshape(-1)
        for p in plan["passes"]:
            assert p["taps"].dtype == np.uint32 and p["wids"].dtype == np.uint32 and p["taps"].shape == p["wids"].shape == (p["count"], p["taps"].shape[1])
            assert int(p["taps"].max()) < data.size
            data = np.sum(data[p["taps"].astype(np.int64)] * p["values"][p["wids"].astype(np.int64)], axis=1)
        return data

    for order in ("hv", "vh", None):
        whole = fhe.resize_plan(sw, sh, dw, dh, "catmull_rom", channels=ch, order=order)
        assert whole["dst"] == (dw, dh) and whole["order"] == (order or whole["order"])
        assert np.max(np.abs(run(whole, img[whole["source_rows"][0]:sum(whole["source_rows"])]).reshape(dh, dw, ch) - want)) < 1e-9
        for cut in range(1, dh):
            parts = []
            for rows in ((0, cut), (cut, dh)):
                plan = fhe.resize_plan(sw, sh, dw, dh, "catmull_rom", channels=ch, rows=rows, order=order)
                first, cnt = plan["source_rows"]
                live = py[1][rows[0]:rows[1]] != 0.0
                assert first == int(py[0][rows[0]:rows[1]][live].min()) and first + cnt - 1 == int(py[0][rows[0]:rows[1]][live].max())
                parts.append(run(plan, img[first:first + cnt]))
            assert np.max(np.abs(np.concatenate(parts).reshape(dh, dw, ch) - want)) < 1e-9
    assert fhe.resize_plan(128, 64, 64, 64)["order"] == "hv" and fhe.resize_plan(64, 128, 64, 64)["order"] == "vh"      # the smaller intermediate
    assert fhe.resize_plan(128, 128, 64, 64)["order"] == "vh" and fhe.resize_plan(64, 64, 128, 128)["order"] == "vh"     # equal: vertical first
    with pytest.raises(ValueError):
        fhe.resize_plan(7, 6, 4, 9, rows=(3, 3))
