"""GPU: the inverse JPEG steps -- fhe_idct8x8_dequant and fhe_ycc_to_rgb_blocks -- bit for bit against their op-by-op
specification on the CPU oracle (tests/idct_oracle.py) and on the GPU Evaluator, and decrypted round trips
(rgb_to_ycc -> dct8x8_quant -> idct8x8_dequant -> ycc_to_rgb) through the Evaluator and through the streaming servers."""
import numpy as np
import pytest

import idct_oracle as io

pytestmark = pytest.mark.gpu

SMALL = dict(n=1024, q=[0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001], t=1 << 14)
P4096_T26 = dict(n=4096, q=[0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001], t=1 << 26)   # room for the chained products of a colour round trip


def _pair(fhe, om, name, **switches):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = SMALL if name == "SMALL" else om.PRESETS[name]
    return fhe.SEALContext(p["n"], p["q"], p["t"], switches=switches or None), om.Oracle(p["n"], p["q"], p["t"])


@pytest.mark.parametrize("quant", ["YQT", None])
@pytest.mark.parametrize("preset,switches", [("SMALL", {}), ("P4096", {}), ("P8192", {}), ("SEAL23_4096", {}),
                                             ("P4096", {"FHE_DCT_FORCE_U64": "1"}), ("P8192", {"FHE_NTT_NOPM": "1"})])
def test_idct_matches_oracle(fhe, oracle_mod, preset, switches, quant):
    ctx, orc = _pair(fhe, oracle_mod, preset, **switches)
    q = fhe.YQT if quant else None
    blocks = ctx.random_ct(2, 64, seed=fhe.SEED + 5)
    out = fhe.Evaluator(ctx).idct8x8_dequant(fhe.IdctPlan(ctx, q), blocks)
    got, host = fhe.to_host(out), fhe.to_host(blocks)
    ops = io.OracleOps(orc)
    assert np.array_equal(got[1], ops.idct_block(host[1], q))


def test_idct_in_place_equals_out_of_place(fhe, oracle_mod):
    ctx, _ = _pair(fhe, oracle_mod, "P4096")
    ev, plan = fhe.Evaluator(ctx), fhe.IdctPlan(ctx, fhe.YQT)
    blocks = ctx.random_ct(3, 64, seed=17)
    ref = fhe.to_host(ev.idct8x8_dequant(plan, blocks))
    ev.idct8x8_dequant(plan, blocks, out=blocks)
    assert np.array_equal(fhe.to_host(blocks), ref)


def test_idct_via_evaluator_calls_matches_fused(fhe, oracle_mod):
    """the spec driven one Evaluator call at a time on the GPU equals the fused launches (and the oracle)"""
    import torch
    ctx, orc = _pair(fhe, oracle_mod, "SMALL")
    ev, enc = fhe.Evaluator(ctx), fhe.FractionalEncoder(ctx)
    blocks = ctx.random_ct(2, 64, seed=321)
    cache = {}

    def M(x, v):
        if v not in cache:
            cache[v] = fhe.PreparedPlain(ctx, enc.encode(v))
        return ev.multiply_plain(x, cache[v])

    data = io.idct_block(ev.add, ev.sub, M, [blocks[:, i].contiguous() for i in range(64)], fhe.YQT)
    stepwise = fhe.to_host(torch.stack(data, dim=1))
    fused = fhe.to_host(ev.idct8x8_dequant(fhe.IdctPlan(ctx, fhe.YQT), blocks))
    assert np.array_equal(stepwise, fused)
    assert np.array_equal(fused[0], io.OracleOps(orc).idct_block(fhe.to_host(blocks)[0], fhe.YQT))


@pytest.mark.parametrize("switches", [{}, {"FHE_DCT_FORCE_U64": "1"}])
def test_idct_launch_chunks_and_empty_batch(fhe, oracle_mod, switches):
    """4097 blocks: on the fused pair 16 waves of 256 blocks and a partial last wave of one, on the general path (forced)
    one 4096-block chunk and a one-block tail.  Blocks either side equal their own single-block runs; an empty batch is a no-op"""
    import torch
    ctx, _ = _pair(fhe, oracle_mod, "SMALL", **switches)
    ev, plan = fhe.Evaluator(ctx), fhe.IdctPlan(ctx, fhe.YQT)
    blocks = ctx.random_ct(4097, 64, seed=99)
    out = ev.idct8x8_dequant(plan, blocks)
    for b in (0, 4095, 4096):
        one = ev.idct8x8_dequant(plan, blocks[b:b + 1].contiguous())
        assert torch.equal(out[b:b + 1], one), b
    del out, blocks
    empty = torch.empty((0, 64, 2, ctx.k, ctx.n), dtype=torch.int64, device=ctx.device)
    assert ev.idct8x8_dequant(plan, empty).shape == empty.shape
    e3 = torch.empty((0, 3, 64, 2, ctx.k, ctx.n), dtype=torch.int64, device=ctx.device)
    assert ev.ycc_to_rgb_blocks(e3).shape == e3.shape
    torch.cuda.synchronize()


def test_idct_fused_pair_equals_general_path(fhe, oracle_mod):
    """P4096 runs k_idct_rows + k_idct_cols; FHE_DCT_FORCE_U64=1 the general path: same bits, on more blocks than one wave"""
    ctx, _ = _pair(fhe, oracle_mod, "P4096")
    assert fhe._lib.load().fhe_dct_path(ctx.h) == 1
    alt, _ = _pair(fhe, oracle_mod, "P4096", FHE_DCT_FORCE_U64="1")
    blocks = ctx.random_ct(300, 64, seed=77)
    a = fhe.Evaluator(ctx).idct8x8_dequant(fhe.IdctPlan(ctx, fhe.YQT), blocks)
    b = fhe.Evaluator(alt).idct8x8_dequant(fhe.IdctPlan(alt, fhe.YQT), blocks)
    assert bool((a == b).all())


def test_idct_refuses_zero_quant(fhe, oracle_mod):
    ctx, _ = _pair(fhe, oracle_mod, "SMALL")
    q = list(fhe.YQT)
    q[9] = 0
    with pytest.raises(fhe.FheError):
        fhe.IdctPlan(ctx, q)


@pytest.mark.parametrize("preset,switches", [("SMALL", {}), ("P4096", {}), ("P8192", {}), ("SEAL23_4096", {}),
                                             ("P4096", {"FHE_DCT_FORCE_U64": "1"})])
def test_ycc_to_rgb_blocks_matches_oracle(fhe, oracle_mod, preset, switches):
    ctx, orc = _pair(fhe, oracle_mod, preset, **switches)
    blocks = ctx.random_ct(2, 3, 64, seed=fhe.SEED + 9)
    host = fhe.to_host(blocks)
    fhe.Evaluator(ctx).ycc_to_rgb_blocks(blocks)
    got = fhe.to_host(blocks)
    ops = io.OracleOps(orc)
    assert np.array_equal(got[1], ops.ycc_to_rgb_block(host[1]))


def _encrypted_rgb_block(orc, pk, pixels, seed):
    """pixels [3][64] -> [3][64][2][k][n] fresh encryptions"""
    out = np.empty((3, 64, 2, orc.k, orc.n), dtype=np.uint64)
    for c in range(3):
        for i in range(64):
            out[c, i] = orc.encrypt(pk, orc.encode(float(pixels[c, i])), seed=seed + 64 * c + i)
    return out


def _decrypt_block(orc, sk, cts):
    vals = np.empty(cts.shape[:2])
    budget = 1 << 30
    for c in range(cts.shape[0]):
        for i in range(cts.shape[1]):
            plain, b = orc.decrypt(sk, cts[c, i])
            vals[c, i] = orc.decode(plain)
            budget = min(budget, b)
    return vals, budget


def test_dct_roundtrip_without_colour_at_t22(fhe, oracle_mod):
    """forward DCT + quant, then dequant + inverse DCT, on one channel-block at t = 2^22 (the limit without the colour steps)"""
    n, q = 4096, [0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001]
    ctx, orc = fhe.SEALContext(n, q, 1 << 22), oracle_mod.Oracle(n, q, 1 << 22)
    sk, pk = orc.keygen(seed=6)
    pix = np.random.default_rng(22).integers(-128, 128, size=(1, 64)).astype(np.float64)
    cts = np.stack([orc.encrypt(pk, orc.encode(float(v)), seed=900 + i) for i, v in enumerate(pix[0])])
    ev = fhe.Evaluator(ctx)
    blocks = fhe.to_device(cts[None], ctx.device)
    back = ev.idct8x8_dequant(fhe.IdctPlan(ctx, fhe.YQT), ev.dct8x8_quant(fhe.DctPlan(ctx, fhe.YQT), blocks))
    got, budget = _decrypt_block(orc, sk, fhe.to_host(back))
    assert np.max(np.abs(got - pix)) < 1e-3
    assert budget > 0


def test_facade_program_equals_python_path(fhe, oracle_mod, tmp_path):
    """seal/idct_check (seal::hip::idct8x8_dequant + ycc_to_rgb_blocks, built against libfhe_hip.so) on two colour blocks equals
    Evaluator.idct8x8_dequant + ycc_to_rgb_blocks on the same ciphertexts"""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(fhe.LIB_PATH), "seal", "idct_check")
    assert os.path.exists(exe), "build() makes seal/idct_check"
    ctx, _ = _pair(fhe, oracle_mod, "P4096")
    srv = fhe.server
    blocks = ctx.random_ct(2, 3, 64, seed=4242)
    host = fhe.to_host(blocks)
    fin, fout = tmp_path / "in.ct", tmp_path / "out.ct"
    with open(fin, "wb") as f:
        for ct in host.reshape(-1, 2, ctx.k, ctx.n):
            srv.write_ciphertext(f, ct)
    r = subprocess.run([exe, str(fin), str(fout), "2", "1", str(ctx.n), str(ctx.t)] + [hex(x) for x in ctx.q],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.zeros_like(host)
    flat = got.reshape(-1, 2, ctx.k, ctx.n)
    with open(fout, "rb") as f:
        for i in range(flat.shape[0]):
            srv.read_ciphertext_into(f, flat[i])
        assert f.read(1) == b""
    ev = fhe.Evaluator(ctx)
    out = ev.idct8x8_dequant(fhe.IdctPlan(ctx, fhe.YQT), blocks.view(6, 64, 2, ctx.k, ctx.n))
    ev.ycc_to_rgb_blocks(out.view(2, 3, 64, 2, ctx.k, ctx.n))
    assert np.array_equal(got, fhe.to_host(out).reshape(host.shape))


@pytest.fixture(scope="module")
def roundtrip(fhe, oracle_mod):
    p = P4096_T26
    ctx, orc = fhe.SEALContext(p["n"], p["q"], p["t"]), oracle_mod.Oracle(p["n"], p["q"], p["t"])
    sk, pk = orc.keygen(seed=5)
    pixels = np.random.default_rng(2026).integers(0, 256, size=(3, 64)).astype(np.float64)
    return ctx, orc, sk, _encrypted_rgb_block(orc, pk, pixels, 500), pixels


def test_roundtrip_through_evaluator_decrypts_to_pixels(fhe, roundtrip):
    ctx, orc, sk, cts, pixels = roundtrip
    ev = fhe.Evaluator(ctx)
    blocks = fhe.to_device(cts[None], ctx.device)
    ev.rgb_to_ycc_blocks(blocks)
    coeffs = ev.dct8x8_quant(fhe.DctPlan(ctx, fhe.YQT), blocks.view(3, 64, 2, ctx.k, ctx.n))
    back = ev.idct8x8_dequant(fhe.IdctPlan(ctx, fhe.YQT), coeffs)
    ev.ycc_to_rgb_blocks(back.view(1, 3, 64, 2, ctx.k, ctx.n))
    got, budget = _decrypt_block(orc, sk, fhe.to_host(back))
    assert np.max(np.abs(got - pixels)) < 1e-3
    assert budget > 0


def test_roundtrip_through_streaming_servers(fhe, roundtrip, tmp_path):
    ctx, orc, sk, cts, pixels = roundtrip
    srv = fhe.server
    fin, fmid, fout = tmp_path / "rgb.ct", tmp_path / "coeffs.ct", tmp_path / "back.ct"
    with open(fin, "wb") as f:
        for c in range(3):
            for i in range(64):
                srv.write_ciphertext(f, cts[c, i])
    assert srv.server_jpeg(ctx, str(fin), str(fmid), 1, quant=list(fhe.YQT)) == 1
    assert srv.server_jpeg_decompress(ctx, str(fmid), str(fout), 1, quant=list(fhe.YQT)) == 1
    back = np.zeros_like(cts)
    with open(fout, "rb") as f:
        for c in range(3):
            for i in range(64):
                srv.read_ciphertext_into(f, back[c, i])
        assert f.read(1) == b""
    got, budget = _decrypt_block(orc, sk, back)
    assert np.max(np.abs(got - pixels)) < 1e-3
    assert budget > 0
