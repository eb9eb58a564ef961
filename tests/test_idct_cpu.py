"""CPU: the inverse JPEG steps (dequantisation + 8x8 IDCT, YCbCr -> RGB) -- the oracle composition of their specification
inverts the float DCT, the library exports the new entry points, and the Python wrappers refuse bad operands before any
launch.  The GPU kernels are compared with these compositions bit for bit in tests/test_gpu_idct.py."""
import ctypes as C
import re
import types

import numpy as np
import pytest

import idct_oracle as io

P4096 = dict(n=4096, q=[0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001], t=1 << 14)
NEW_SYMBOLS = ("fhe_idct_plan_create", "fhe_idct_plan_destroy", "fhe_idct8x8_scratch_bytes", "fhe_idct8x8_dequant", "fhe_ycc_to_rgb_blocks")


@pytest.fixture(scope="module")
def p4096(oracle_mod):
    orc = oracle_mod.Oracle(P4096["n"], P4096["q"], P4096["t"])
    sk, pk = orc.keygen(seed=3)
    return orc, sk, pk


def _encrypt_values(orc, pk, values, seed):
    return [orc.encrypt(pk, orc.encode(float(v)), seed=seed + i) for i, v in enumerate(values)]


def _decrypt_values(orc, sk, cts):
    vals, budgets = [], []
    for ct in cts:
        plain, budget = orc.decrypt(sk, ct)
        vals.append(orc.decode(plain))
        budgets.append(budget)
    return np.array(vals), min(budgets)


def test_oracle_idct_inverts_float_dct(p4096, oracle_mod):
    """fresh encryptions of float DCT coefficients / Q -> dequantise + IDCT -> the pixels (t = 2^14 holds one direction)"""
    orc, sk, pk = p4096
    pix = np.random.default_rng(7).uniform(-128, 127, size=64)
    coeffs = io.fdct_float(pix).reshape(64) / np.array(oracle_mod.YQT, dtype=np.float64)
    ops = io.OracleOps(orc)
    out = io.idct_block(ops.A, ops.S, ops.M, _encrypt_values(orc, pk, coeffs, 100), oracle_mod.YQT)
    got, budget = _decrypt_values(orc, sk, out)
    assert np.max(np.abs(got - pix)) < 1e-6
    assert budget > 0


def test_oracle_ycc_to_rgb_inverts_rgb_to_ycc(p4096):
    orc, sk, pk = p4096
    rgb = np.random.default_rng(8).uniform(0, 255, size=(3, 4))
    cts = [_encrypt_values(orc, pk, rgb[c], 1000 + 100 * c) for c in range(3)]
    ops = io.OracleOps(orc)
    for i in range(4):
        y, cb, cr = orc.rgb_to_ycc(cts[0][i], cts[1][i], cts[2][i])
        back = io.ycc_to_rgb(ops.A, ops.S, ops.M, ops.AP, y, cb, cr)
        got, budget = _decrypt_values(orc, sk, back)
        assert np.max(np.abs(got - rgb[:, i])) < 1e-3
        assert budget > 0


def test_float_dct_model_matches_the_line_constants():
    """fdct_float (orthonormal) is what the LL&M line with its 0.125 scale computes: its transpose inverts it"""
    x = np.random.default_rng(1).uniform(-1, 1, size=(8, 8))
    k = np.arange(8)
    Cm = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) / 2
    Cm[0] /= np.sqrt(2)
    assert np.allclose(Cm.T @ io.fdct_float(x) @ Cm, x)


def test_library_exports_the_inverse_entry_points(fhe):
    lib = C.CDLL(fhe.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in fhe._lib.SIGNATURES, name
    hdr = open(fhe.HEADER_PATH).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name


def test_abi_version_unchanged(fhe):
    """entry points were added, none changed: the version stays 4"""
    assert "#define FHE_ABI_VERSION 4" in open(fhe.HEADER_PATH).read()


def _fake_ctx(n=64, k=3):
    import torch
    return types.SimpleNamespace(n=n, k=k, device=torch.device("cpu"), h=None)


def test_idct_wrapper_refuses_bad_operands(fhe):
    import torch
    ctx = _fake_ctx()
    ev = fhe.Evaluator(ctx)
    plan = types.SimpleNamespace(ctx=ctx, h=None)
    good = torch.zeros(2, 64, 2, ctx.k, ctx.n, dtype=torch.int64)
    for bad in (torch.zeros(2, 63, 2, ctx.k, ctx.n, dtype=torch.int64),            # 63 ciphertexts per block
                torch.zeros(2, 64, 3, ctx.k, ctx.n, dtype=torch.int64),            # size 3
                torch.zeros(2, 64, 2, ctx.k, ctx.n, dtype=torch.int32),            # dtype
                good.transpose(0, 1),                                              # not contiguous (and wrong shape)
                torch.zeros(64 * 2 * ctx.k * ctx.n, dtype=torch.int64)):           # flat
        with pytest.raises(ValueError):
            ev.idct8x8_dequant(plan, bad)
    with pytest.raises(ValueError):
        ev.idct8x8_dequant(plan, good, out=torch.zeros(1, 64, 2, ctx.k, ctx.n, dtype=torch.int64))
    with pytest.raises(ValueError):
        ev.idct8x8_dequant(types.SimpleNamespace(ctx=_fake_ctx(n=128), h=None), good)
    with pytest.raises(ValueError):
        fhe.IdctPlan(ctx, quant=[1.0] * 63)


def test_ycc_to_rgb_wrapper_refuses_bad_operands(fhe):
    import torch
    ctx = _fake_ctx()
    ev = fhe.Evaluator(ctx)
    for bad in (torch.zeros(2, 64, 2, ctx.k, ctx.n, dtype=torch.int64),            # no channel axis
                torch.zeros(2, 2, 64, 2, ctx.k, ctx.n, dtype=torch.int64),         # two channels
                torch.zeros(2, 3, 64, 2, ctx.k, ctx.n, dtype=torch.float64),
                torch.zeros(2, 3, 64, 2, ctx.k, 2 * ctx.n, dtype=torch.int64)):
        with pytest.raises(ValueError):
            ev.ycc_to_rgb_blocks(bad)
