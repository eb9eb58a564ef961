"""GPU parity: every C-ABI entry point against the CPU oracle, bit for bit.

All tests call libfhe_hip.so through the C ABI (ctypes) and compare with oracle/ on the same
seeded inputs.  Integer work => the bar is exact equality.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL = dict(n=1024, q=[0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001], t=1 << 14)


def _pair(fhe, om, name):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = SMALL if name == "SMALL" else om.PRESETS[name]
    return fhe.SEALContext(p["n"], p["q"], p["t"]), om.Oracle(p["n"], p["q"], p["t"])


def _variant(fhe, ctx, **switches):
    """a second context on the same parameters with experiment switches set: the library reads them once, in
    fhe_ctx_create (csrc/internal.h FheOptions); device tensors, plans and prepared plaintexts are interchangeable"""
    return fhe.SEALContext(ctx.n, ctx.q, ctx.t, switches=switches)


@pytest.fixture(scope="module", params=["SMALL", "P4096", "P8192"])
def pair(request, fhe, oracle_mod):
    return _pair(fhe, oracle_mod, request.param)


def test_fill_random_matches_oracle(pair, fhe):
    ctx, orc = pair
    g = fhe.to_host(ctx.random_ct(3, seed=fhe.SEED, first_index=17))
    o = orc.random_ct(3, seed=fhe.SEED, first_index=17)
    assert np.array_equal(g, o)


def test_add_sub_negate(pair, fhe):
    ctx, orc = pair
    ev = fhe.Evaluator(ctx)
    a, b = ctx.random_ct(4, seed=1), ctx.random_ct(4, seed=2)
    ha, hb = fhe.to_host(a), fhe.to_host(b)
    for i in range(4):
        assert np.array_equal(fhe.to_host(ev.add(a, b))[i], orc.add(ha[i], hb[i]))
        assert np.array_equal(fhe.to_host(ev.sub(a, b))[i], orc.sub(ha[i], hb[i]))
        assert np.array_equal(fhe.to_host(ev.negate(a))[i], orc.negate(ha[i]))


def test_add_sub_edge_values(pair, fhe):
    """0, q-1 and equal operands: the modular wrap cases."""
    ctx, orc = pair
    ev = fhe.Evaluator(ctx)
    a = np.zeros((2, ctx.k, ctx.n), dtype=np.uint64)
    b = np.zeros_like(a)
    for i, q in enumerate(ctx.q):
        a[0, i, :] = q - 1
        b[0, i, ::2] = q - 1
        b[1, i, 1::2] = 1
    da, db = fhe.to_device(a), fhe.to_device(b)
    assert np.array_equal(fhe.to_host(ev.add(da, db)), orc.add(a, b))
    assert np.array_equal(fhe.to_host(ev.sub(da, db)), orc.sub(a, b))
    assert np.array_equal(fhe.to_host(ev.sub(db, da)), orc.sub(b, a))
    assert np.array_equal(fhe.to_host(ev.negate(db)), orc.negate(b))


def test_add_unequal_sizes(pair, fhe):
    ctx, orc = pair
    ev = fhe.Evaluator(ctx)
    a, b = ctx.random_ct(size=2, seed=3), ctx.random_ct(size=4, seed=4)
    ha, hb = fhe.to_host(a), fhe.to_host(b)
    assert np.array_equal(fhe.to_host(ev.add(a, b)), orc.add(ha, hb))
    assert np.array_equal(fhe.to_host(ev.sub(a, b)), orc.sub(ha, hb))
    assert np.array_equal(fhe.to_host(ev.sub(b, a)), orc.sub(hb, ha))


def test_ntt_roundtrip_and_product(pair, fhe):
    """inverse(forward(x)) == x, and forward/dyadic/inverse == the oracle's ring product."""
    ctx, orc = pair
    ev = fhe.Evaluator(ctx)
    a, b = ctx.random_ct(2, seed=5), ctx.random_ct(2, seed=6)
    fa, fb = ev.ntt_forward(a), ev.ntt_forward(b)
    assert np.array_equal(fhe.to_host(ev.ntt_inverse(fa)), fhe.to_host(a))
    prod = fhe.to_host(ev.ntt_inverse(ev.dyadic_multiply(fa, fb)))
    ha, hb = fhe.to_host(a), fhe.to_host(b)
    for c in range(2):
        for j in range(2):
            for i, q in enumerate(ctx.q):
                x, y = orc.ntt_fwd(ha[c, j, i], i), orc.ntt_fwd(hb[c, j, i], i)
                ref = orc.ntt_inv(np.array([(int(u) * int(v)) % q for u, v in zip(x, y)], dtype=np.uint64), i)
                assert np.array_equal(prod[c, j, i], ref)
    # the forward transform is a permutation of the oracle's (slot order is internal)
    h = fhe.to_host(fa)
    assert np.array_equal(np.sort(h[0, 0, 0]), np.sort(orc.ntt_fwd(ha[0, 0, 0], 0)))


CONSTS = [0.541196100, -1.847759065, 0.125, 3.0, 128.0, 1 / 16.0, -0.168736, 1.0, -1.0, 0.0, 1 / 99.0, -4.71238898038469]


def test_encoder_matches_oracle(pair, fhe):
    ctx, orc = pair
    enc = fhe.FractionalEncoder(ctx)
    for v in CONSTS + [255.0, -255.75, 1e-9, 12345.678]:
        assert np.array_equal(enc.encode(v), orc.encode(v)), v
        assert enc.decode(enc.encode(v)) == orc.decode(orc.encode(v))


def test_multiply_plain(pair, fhe):
    ctx, orc = pair
    ev, enc = fhe.Evaluator(ctx), fhe.FractionalEncoder(ctx)
    a = ctx.random_ct(2, seed=7)
    ha = fhe.to_host(a)
    for v in CONSTS:
        got = fhe.to_host(ev.multiply_plain(a, enc.encode(v)))
        for i in range(2):
            assert np.array_equal(got[i], orc.multiply_plain(ha[i], orc.encode(v))), v


def test_multiply_plain_dense_plaintext(pair, fhe):
    """a plaintext with every coefficient set, including upper-half (negative) values"""
    ctx, orc = pair
    ev = fhe.Evaluator(ctx)
    rng = np.random.default_rng(5)
    plain = rng.integers(0, ctx.t, size=ctx.n, dtype=np.uint64)
    plain[0], plain[1], plain[2] = ctx.t - 1, (ctx.t + 1) // 2, (ctx.t + 1) // 2 - 1
    a = ctx.random_ct(size=3, seed=8)
    assert np.array_equal(fhe.to_host(ev.multiply_plain(a, plain)), orc.multiply_plain(fhe.to_host(a), plain))


def test_add_sub_plain(pair, fhe):
    ctx, orc = pair
    ev, enc = fhe.Evaluator(ctx), fhe.FractionalEncoder(ctx)
    a = ctx.random_ct(3, seed=9)
    ha = fhe.to_host(a)
    for v in [128.0, -0.5, 1.0, -4.71238898038469, 3.0]:
        p = enc.encode(v)
        ga, gs = fhe.to_host(ev.add_plain(a, p)), fhe.to_host(ev.sub_plain(a, p))
        for i in range(3):
            assert np.array_equal(ga[i], orc.add_plain(ha[i], p)), v
            assert np.array_equal(gs[i], orc.sub_plain(ha[i], p)), v


@pytest.mark.parametrize("preset,n_blocks", [("SMALL", 3), ("P4096", 2)])
def test_dct_quant_fused_vs_op_at_a_time(fhe, oracle_mod, preset, n_blocks):
    """fused block circuit == the reference's 832 Evaluator calls, bit for bit"""
    ctx, orc = _pair(fhe, oracle_mod, preset)
    ev = fhe.Evaluator(ctx)
    blocks = ctx.random_ct(n_blocks, 64, seed=fhe.SEED)
    plan = fhe.DctPlan(ctx, fhe.YQT)
    got = fhe.to_host(ev.dct8x8_quant(plan, blocks))
    hb = fhe.to_host(blocks)
    for b in range(n_blocks):
        assert np.array_equal(got[b], orc.dct_quant(hb[b], fhe.YQT)), b


def test_dct_without_quant(fhe, oracle_mod):
    ctx, orc = _pair(fhe, oracle_mod, "SMALL")
    ev = fhe.Evaluator(ctx)
    blocks = ctx.random_ct(1, 64, seed=77)
    got = fhe.to_host(ev.dct8x8_quant(fhe.DctPlan(ctx, None), blocks))
    assert np.array_equal(got[0], orc.encrypted_dct(fhe.to_host(blocks)[0]))


def test_dct_via_evaluator_calls_matches_fused(fhe, oracle_mod):
    """drive the GPU one Evaluator call at a time (the reference's shape) and compare with the fused kernel"""
    ctx, orc = _pair(fhe, oracle_mod, "SMALL")
    ev, enc = fhe.Evaluator(ctx), fhe.FractionalEncoder(ctx)
    blocks = ctx.random_ct(2, 64, seed=123)
    cache = {}

    def P(v):
        if v not in cache:
            cache[v] = fhe.PreparedPlain(ctx, enc.encode(v))
        return cache[v]

    def line(d, scale):
        A, S, M = ev.add, ev.sub, ev.multiply_plain
        t0, t7, t1, t6 = A(d[0], d[7]), S(d[0], d[7]), A(d[1], d[6]), S(d[1], d[6])
        t2, t5, t3, t4 = A(d[2], d[5]), S(d[2], d[5]), A(d[3], d[4]), S(d[3], d[4])
        t10, t13, t11, t12 = A(t0, t3), S(t0, t3), A(t1, t2), S(t1, t2)
        o = [None] * 8
        o[0], o[4] = A(t10, t11), S(t10, t11)
        z1 = M(A(t12, t13), P(0.541196100))
        o[2], o[6] = A(z1, M(t13, P(0.765366865))), A(z1, M(t12, P(-1.847759065)))
        z1, z2, z3, z4 = A(t4, t7), A(t5, t6), A(t4, t6), A(t5, t7)
        z5 = M(A(z3, z4), P(1.175875602))
        t4, t5, t6, t7 = M(t4, P(0.298631336)), M(t5, P(2.053119869)), M(t6, P(3.072711026)), M(t7, P(1.501321110))
        z1, z2 = M(z1, P(-0.899976223)), M(z2, P(-2.562915447))
        z3, z4 = A(M(z3, P(-1.961570560)), z5), A(M(z4, P(-0.390180644)), z5)
        o[7], o[5], o[3], o[1] = A(A(t4, z1), z3), A(A(t5, z2), z4), A(A(t6, z2), z3), A(A(t7, z1), z4)
        return [M(x, P(0.125)) for x in o] if scale else o

    data = [blocks[:, i].contiguous() for i in range(64)]      # each [n_blocks, 2, k, n]
    for r in range(8):
        data[8 * r:8 * r + 8] = line(data[8 * r:8 * r + 8], False)
    for c in range(8):
        col = line([data[c + 8 * i] for i in range(8)], True)
        for i in range(8):
            data[c + 8 * i] = col[i]
    data = [ev.multiply_plain(d, P(1 / qv)) for d, qv in zip(data, fhe.YQT)]
    import torch
    stepwise = fhe.to_host(torch.stack(data, dim=1))
    fused = fhe.to_host(ev.dct8x8_quant(fhe.DctPlan(ctx, fhe.YQT), blocks))
    assert np.array_equal(stepwise, fused)
    assert np.array_equal(fused[1], orc.dct_quant(fhe.to_host(blocks)[1], fhe.YQT))


@pytest.mark.parametrize("preset", ["SMALL", "P4096", "P8192", "SEAL23_4096"])
def test_rgb_to_ycc(fhe, oracle_mod, preset):
    """SMALL runs the general u64 kernel, P8192 / SEAL23_4096 its pseudo-Mersenne form, P4096 the fused FP64 kernel
    (csrc/dct_fused.hip)."""
    ctx, orc = _pair(fhe, oracle_mod, preset)
    ev = fhe.Evaluator(ctx)
    r, g, b = ctx.random_ct(3, seed=31), ctx.random_ct(3, seed=32), ctx.random_ct(3, seed=33)
    hr, hg, hb = fhe.to_host(r).copy(), fhe.to_host(g).copy(), fhe.to_host(b).copy()
    ev.rgb_to_ycc(r, g, b)
    for i in range(3):
        y, u, v = orc.rgb_to_ycc(hr[i], hg[i], hb[i])
        assert np.array_equal(fhe.to_host(r)[i], y)
        assert np.array_equal(fhe.to_host(g)[i], u)
        assert np.array_equal(fhe.to_host(b)[i], v)


@pytest.mark.parametrize("preset", ["P4096", "SEAL23_4096", "P8192"])
def test_rgb_to_ycc_blocks_layout_equals_planes(fhe, preset):
    """fhe_rgb_to_ycc_blocks (the stream layout [blocks][3][64][2][k][n], planes 64 ciphertexts apart inside a block) gives
    the same ciphertexts as fhe_rgb_to_ycc on three separate planes -- the FP64 kernel (P4096) and the three-launch
    pseudo-Mersenne path (SEAL23_4096, P8192) with its strided plane addressing."""
    import torch
    ctx = fhe.SEALContext.preset(preset)
    ev = fhe.Evaluator(ctx)
    blocks = ctx.random_ct(2, 3, 64, seed=77)                   # [2, 3, 64, 2, k, n]
    r, g, b = (blocks[:, p].reshape(128, 2, ctx.k, ctx.n).clone() for p in range(3))
    ev.rgb_to_ycc(r, g, b)
    ev.rgb_to_ycc_blocks(blocks)
    for p, want in enumerate((r, g, b)):
        assert torch.equal(blocks[:, p].reshape(128, 2, ctx.k, ctx.n), want), (preset, p)


def test_rgb_to_ycc_fp64_path_equals_u64_path_and_extremes(fhe, oracle_mod, monkeypatch):
    """P4096: the FP64 kernel against the u64 kernel on 40 pixels, including all-(q-1) and all-zero
    residues (largest magnitudes the exact FP64 products see), and repeated calls (cached constants)."""
    import torch
    ctx, orc = _pair(fhe, oracle_mod, "P4096")
    ev = fhe.Evaluator(ctx)
    base = [ctx.random_ct(40, seed=71 + i) for i in range(3)]
    qm1 = torch.tensor([q - 1 for q in ctx.q], dtype=torch.int64, device=base[0].device).view(1, ctx.k, 1)
    for t in base:
        t[0] = qm1.expand(2, ctx.k, ctx.n)
        t[1] = 0
    base[1][2] = qm1.expand(2, ctx.k, ctx.n)
    fast = [t.clone() for t in base]
    ev.rgb_to_ycc(*fast)
    again = [t.clone() for t in base]
    ev.rgb_to_ycc(*again)
    slow = [t.clone() for t in base]
    fhe.Evaluator(_variant(fhe, ctx, FHE_DCT_FORCE_U64=1)).rgb_to_ycc(*slow)
    for a, b, c in zip(fast, slow, again):
        assert torch.equal(a, b) and torch.equal(a, c)
    for i in (0, 1, 2):
        y, u, v = orc.rgb_to_ycc(*(fhe.to_host(t)[i] for t in base))
        assert np.array_equal(fhe.to_host(fast[0])[i], y)
        assert np.array_equal(fhe.to_host(fast[1])[i], u)
        assert np.array_equal(fhe.to_host(fast[2])[i], v)


@pytest.mark.parametrize("preset,switches", [("SEAL23_4096", {"FHE_NTT_NOPM": 1}), ("P8192", {"FHE_NTT_NOPM": 1}), ("P4096", {"FHE_DCT_FORCE_U64": 1})])
def test_rgb_to_ycc_one_launch_kernel_back_to_back_inverse_transforms(fhe, oracle_mod, preset, switches):
    """k_rgb2ycc (the path of bases that are not pseudo-Mersenne and of FHE_NTT_NOPM=1) runs three inverse transforms back to back on
    ONE LDS buffer; an inverse transform ends with a transpose that reads across waves, the next one opens with a wave-local write
    (csrc/ntt_core.h, CONTRACT) -- the ntt_lds_release() between them is what this stresses: 512 pixels x 4 rounds at n = 4096 / 8192
    (8 and 16 waves per workgroup, thousands of workgroups in flight), every round bit-equal to the default three-launch / FP64 path,
    sampled pixels equal to the oracle."""
    import torch
    ctx, orc = _pair(fhe, oracle_mod, preset)
    alt = _variant(fhe, ctx, **switches)
    ev, ev2 = fhe.Evaluator(ctx), fhe.Evaluator(alt)
    base = [ctx.random_ct(512, seed=301 + i) for i in range(3)]
    want = [t.clone() for t in base]
    ev.rgb_to_ycc(*want)
    for rnd in range(4):
        got = [t.clone() for t in base]
        ev2.rgb_to_ycc(*got)
        for p, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (preset, rnd, p)
    for i in (0, 255, 511):
        y, u, v = orc.rgb_to_ycc(*(fhe.to_host(t[i:i + 1])[0] for t in base))
        assert np.array_equal(fhe.to_host(want[0][i:i + 1])[0], y) and np.array_equal(fhe.to_host(want[1][i:i + 1])[0], u)
        assert np.array_equal(fhe.to_host(want[2][i:i + 1])[0], v)


def test_dct_known_answer_through_decrypt(fhe, oracle_mod):
    """decrypt(GPU circuit(encrypt(pixels))) == the plaintext DCT of homo/fhe_image.h:400-484 / quant"""
    from oracle import bigint_model as bm
    ctx, orc = _pair(fhe, oracle_mod, "P4096")
    ev = fhe.Evaluator(ctx)
    sk, pk = orc.keygen(42)
    vals = [float((37 * x + 101 * y + 13) % 256) - 128.0 for y in range(8) for x in range(8)]
    blk = np.stack([orc.encrypt(pk, orc.encode(v), seed=1000 + i) for i, v in enumerate(vals)])[None]
    out = fhe.to_host(ev.dct8x8_quant(fhe.DctPlan(ctx, fhe.YQT), fhe.to_device(blk)))[0]
    expect = bm.plain_dct(vals)
    for i in range(64):
        plain, budget = orc.decrypt(sk, out[i])
        assert budget > 0
        assert abs(orc.decode(plain) - expect[i] / fhe.YQT[i]) < 1e-6   # tolerance: decode is exact up to double rounding


def test_digest_is_order_independent_and_matches_numpy(fhe, oracle_mod):
    ctx, _ = _pair(fhe, oracle_mod, "SMALL")
    a = ctx.random_ct(2, seed=55)
    h = fhe.to_host(a).ravel()
    M = (1 << 64) - 1

    def sm(x):
        x = (x + 0x9E3779B97F4A7C15) & M
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
        return x ^ (x >> 31)

    ref = 0
    for i, v in enumerate(h[:5000]):
        ref = (ref + sm(int(v) ^ sm(i))) & M
    assert ctx.digest(a.view(-1)[:5000].contiguous()) == ref


@pytest.mark.parametrize("preset,n_blocks", [("P4096", 3), ("SEAL3_8192", 1), ("SEAL23_4096", 3), ("P8192", 2), ("SEAL23_2048", 2)])
def test_dct_fp64_path_equals_u64_path(fhe, oracle_mod, preset, n_blocks, monkeypatch):
    """The fused two-launch kernels -- exact-FP64 (dct_fused.hip, primes below 2^47) or u64 Shoup (dct_u64.hip,
    the 54/55-bit primes of SEAL23_4096 / P8192 / SEAL23_2048) -- and the general three-launch u64 path produce
    identical bytes, equal to the oracle's op-at-a-time evaluation."""
    ctx, orc = _pair(fhe, oracle_mod, preset)
    ev = fhe.Evaluator(ctx)
    blocks = ctx.random_ct(n_blocks, 64, seed=99)
    plan = fhe.DctPlan(ctx, fhe.YQT)
    fused = fhe.to_host(ev.dct8x8_quant(plan, blocks))
    general = fhe.to_host(fhe.Evaluator(_variant(fhe, ctx, FHE_DCT_FORCE_U64=1)).dct8x8_quant(plan, blocks))
    assert np.array_equal(fused, general)
    assert np.array_equal(fused[0], orc.dct_quant(fhe.to_host(blocks)[0], fhe.YQT))


@pytest.mark.parametrize("preset", ["P4096", "SEAL3_8192"])
def test_dct_extreme_residues(fhe, oracle_mod, preset):
    """all-(q-1) and all-zero inputs: largest magnitudes through the lazy FP64 pipeline (36-bit primes with the packed
    intermediate; 43/44-bit primes with the reducing variant at 8 coefficients per thread, n = 8192)"""
    ctx, orc = _pair(fhe, oracle_mod, preset)
    ev = fhe.Evaluator(ctx)
    blk = np.zeros((1, 64, 2, ctx.k, ctx.n), dtype=np.uint64)
    for i, q in enumerate(ctx.q):
        blk[0, :, :, i, :] = q - 1
    blk[0, 5] = 0
    out = fhe.to_host(ev.dct8x8_quant(fhe.DctPlan(ctx, fhe.YQT), fhe.to_device(blk)))
    assert np.array_equal(out[0], orc.dct_quant(blk[0], fhe.YQT))


def test_dct_fp64_fused_at_n2048(fhe, oracle_mod, monkeypatch):
    """n = 2048 with primes below 2^47 (the P4096 primes are = 1 mod 8192, so they serve n = 2048 too): the fused FP64 pair
    with 8 coefficients per thread and a last register pass of two stages; random and all-(q-1) blocks against the oracle
    and against the general three-launch path"""
    q = [0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001]
    ctx, orc = fhe.SEALContext(2048, q, 1 << 14), oracle_mod.Oracle(2048, q, 1 << 14)
    ev = fhe.Evaluator(ctx)
    blk = fhe.to_host(ctx.random_ct(3, 64, seed=77))
    for i, qi in enumerate(q):
        blk[1, :, :, i, :] = qi - 1
    blk[1, 3] = 0
    d = fhe.to_device(blk)
    plan = fhe.DctPlan(ctx, fhe.YQT)
    out = fhe.to_host(ev.dct8x8_quant(plan, d))
    for b in range(3):
        assert np.array_equal(out[b], orc.dct_quant(blk[b], fhe.YQT)), b
    ctx_u64 = _variant(fhe, ctx, FHE_DCT_FORCE_U64=1)
    assert np.array_equal(fhe.to_host(fhe.Evaluator(ctx_u64).dct8x8_quant(fhe.DctPlan(ctx_u64, fhe.YQT), d)), out)


@pytest.mark.parametrize("preset", ["SEAL23_4096", "P8192"])
def test_dct_extreme_residues_u64_fused(fhe, oracle_mod, preset):
    """all-(q-1) inputs through the lazy ranges of the fused u64 kernels (values up to 128 q before the scale product).  All-(q-1) inputs
    are the largest inputs, not the worst case of those ranges, and meet none of the values the exits are delicate for: prescribed outputs,
    exact zeros, the widest operands and every instantiation are in tests/test_gpu_dct_u64_extremes.py."""
    ctx, orc = _pair(fhe, oracle_mod, preset)
    ev = fhe.Evaluator(ctx)
    blk = np.zeros((1, 64, 2, ctx.k, ctx.n), dtype=np.uint64)
    for i, q in enumerate(ctx.q):
        blk[0, :, :, i, :] = q - 1
    blk[0, 5] = 0
    blk[0, 9, :, :, ::2] = 1
    out = fhe.to_host(ev.dct8x8_quant(fhe.DctPlan(ctx, fhe.YQT), fhe.to_device(blk)))
    assert np.array_equal(out[0], orc.dct_quant(blk[0], fhe.YQT))


def test_fused_dct_matches_bigint_model_golden_n4096(fhe):
    """the HIP fused path against the big-integer model's committed SHA-256 (no oracle in between)"""
    import hashlib
    import os
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dct_quant_n4096_digest.npz"))
    ctx = fhe.SEALContext(int(d["n"]), d["q"].tolist(), int(d["t"]))
    ev = fhe.Evaluator(ctx)
    out = fhe.to_host(ev.dct8x8_quant(fhe.DctPlan(ctx, d["quant"].tolist()), ctx.random_ct(1, 64, seed=fhe.SEED)))[0]
    assert hashlib.sha256(out.tobytes()).hexdigest() == str(d["sha256_dct_quant"])
    assert np.array_equal(out[d["sample_index"]][:, :, :, :16], d["dct_quant_sample"])


def test_full_size_properties_1024_blocks(fhe, oracle_mod):
    """BASELINE.json configs[1] at full size (1024 blocks): size-independent checks.
    (a) linearity: circuit(a + b) == circuit(a) + circuit(b) over all blocks (digest equality);
    (b) every rank-style shard regenerates the same bytes: digest of two halves == digest of the whole;
    (c) sampled blocks bit-equal to the oracle."""
    ctx, orc = _pair(fhe, oracle_mod, "P4096")
    ev = fhe.Evaluator(ctx)
    plan = fhe.DctPlan(ctx, fhe.YQT)
    B = 1024
    a = ctx.random_ct(B, 64, seed=fhe.SEED)
    ca = ev.dct8x8_quant(plan, a)
    wpb = 64 * 2 * ctx.k * ctx.n
    whole = ctx.digest(ca.view(-1))
    halves = (ctx.digest(ca[:512].reshape(-1), 0) + ctx.digest(ca[512:].reshape(-1), 512 * wpb)) & ((1 << 64) - 1)
    assert whole == halves
    for b in (0, 777):
        assert np.array_equal(fhe.to_host(ca[b]), orc.dct_quant(fhe.to_host(a[b]), fhe.YQT))
    # linearity on a 256-block slice (memory: three more 3 GiB tensors)
    bsl = ctx.random_ct(256, 64, seed=12345)
    s = ev.add(a[:256].contiguous(), bsl)
    lhs = ev.dct8x8_quant(plan, s)
    rhs = ev.add(ca[:256].contiguous(), ev.dct8x8_quant(plan, bsl))
    assert ctx.digest(lhs.view(-1)) == ctx.digest(rhs.view(-1))
    import torch
    assert torch.equal(lhs, rhs)


# ---------------------------------------------------------------------------------------------
# ct x ct (BEHZ) and relinearisation
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", ["SMALL", "P4096", "P8192", "SEAL23_4096"])
def test_multiply_square_all_shapes(fhe, oracle_mod, preset):
    """the multiply shapes the reference's circuits exercise: 2x2, square(2),
    2x3, 4x3, 4x2, square(3), batched over two pairs"""
    ctx, orc = _pair(fhe, oracle_mod, preset)
    ev = fhe.Evaluator(ctx)
    a2, b2 = ctx.random_ct(2, size=2, seed=201), ctx.random_ct(2, size=2, seed=202)
    h = fhe.to_host
    ab = ev.multiply(a2, b2)
    for i in range(2):
        assert np.array_equal(h(ab)[i], orc.multiply(h(a2)[i], h(b2)[i]))
    sq = ev.square(a2)
    for i in range(2):
        assert np.array_equal(h(sq)[i], orc.square(h(a2)[i]))
    a4 = ctx.random_ct(2, size=4, seed=203)
    m23, m43, m42 = ev.multiply(a2, ab), ev.multiply(a4, ab), ev.multiply(a4, b2)
    sq3 = ev.square(ab)
    for i in range(2):
        assert np.array_equal(h(m23)[i], orc.multiply(h(a2)[i], h(ab)[i]))
        assert np.array_equal(h(m43)[i], orc.multiply(h(a4)[i], h(ab)[i]))
        assert np.array_equal(h(m42)[i], orc.multiply(h(a4)[i], h(b2)[i]))
        assert np.array_equal(h(sq3)[i], orc.square(h(ab)[i]))
    assert m43.shape[-3] == 6 and sq3.shape[-3] == 5


def test_multiply_large_sizes_decode_shapes(fhe, oracle_mod):
    """(11 x 11) -> 21 and (21 x 2) -> 22: the term/amplitude products of approximated_step"""
    ctx, orc = _pair(fhe, oracle_mod, "SMALL")
    ev = fhe.Evaluator(ctx)
    a, b, c = ctx.random_ct(1, size=11, seed=301), ctx.random_ct(1, size=11, seed=302), ctx.random_ct(1, size=2, seed=303)
    t = ev.multiply(a, b)
    assert t.shape[-3] == 21
    assert np.array_equal(fhe.to_host(t)[0], orc.multiply(fhe.to_host(a)[0], fhe.to_host(b)[0]))
    u = ev.multiply(t, c)
    assert u.shape[-3] == 22
    assert np.array_equal(fhe.to_host(u)[0], orc.multiply(fhe.to_host(t)[0], fhe.to_host(c)[0]))


@pytest.mark.parametrize("size", [12, 13])
def test_multiply_term_limit_of_the_lazy_tensor_sum(fhe, oracle_mod, size):
    """12 x 12 is the largest product whose tensor sums stay unreduced (12 terms of [0, 5q) below 2^64 on a base of 58-bit
    primes), 13 x 13 takes the reduced schedule; operands at q - 1 everywhere put every residue product at its extreme"""
    ctx, orc = _pair(fhe, oracle_mod, "SMALL")
    ev = fhe.Evaluator(ctx)
    a = fhe.to_host(ctx.random_ct(1, size=size, seed=311))
    b = np.zeros_like(a)
    for i, q in enumerate(ctx.q):
        b[0, :, i, :] = q - 1
    for x, y in ((a, a[:, ::-1].copy()), (a, b), (b, b)):
        t = ev.multiply(fhe.to_device(x), fhe.to_device(y))
        assert t.shape[-3] == 2 * size - 1
        assert np.array_equal(fhe.to_host(t)[0], orc.multiply(x[0], y[0]))


def test_multiply_edge_inputs(fhe, oracle_mod):
    """zero, and q - 1 everywhere: the wrap cases of the residue-wise tensor sums.  For the base conversions this is the SMALLEST
    product, not an extreme: q - 1 lifts to the centred value -1, the product is +1 and the fast floor leaves v ~ t / q
    (their extremes: tests/test_gpu_behz_extremes.py)"""
    ctx, orc = _pair(fhe, oracle_mod, "SMALL")
    ev = fhe.Evaluator(ctx)
    a = np.zeros((1, 2, ctx.k, ctx.n), dtype=np.uint64)
    for i, q in enumerate(ctx.q):
        a[0, :, i, :] = q - 1
    z = np.zeros_like(a)
    da, dz = fhe.to_device(a), fhe.to_device(z)
    assert np.array_equal(fhe.to_host(ev.multiply(da, da))[0], orc.multiply(a[0], a[0]))
    assert np.array_equal(fhe.to_host(ev.multiply(da, dz))[0], orc.multiply(a[0], z[0]))
    assert np.array_equal(fhe.to_host(ev.square(da))[0], orc.square(a[0]))


@pytest.mark.parametrize("preset,dbc", [("SMALL", 16), ("SMALL", 30), ("P8192", 30), ("P8192", 60), ("SEAL23_4096", 16)])
def test_relinearize(fhe, oracle_mod, preset, dbc):
    """SMALL: the five-launch Shoup path; P8192 / SEAL23_4096: the three fused pseudo-Mersenne launches (digit extraction
    inside the forward transforms, lazy key products, inverse transform + addition), with digits narrower and -- dbc = 60 --
    wider than the primes."""
    ctx, orc = _pair(fhe, oracle_mod, preset)
    ev = fhe.Evaluator(ctx)
    sk, pk = orc.keygen(77)
    evk = orc.evk_gen(sk, dbc=dbc)                       # oracle NTT form [k][nd][2][k][n]
    coeff = np.zeros_like(evk)
    for idx in np.ndindex(evk.shape[:3]):
        for i in range(ctx.k):
            coeff[idx + (i,)] = orc.ntt_inv(evk[idx + (i,)], i)
    evk_dev = ev.ntt_forward(fhe.to_device(coeff))       # library slot order
    c1 = orc.encrypt(pk, orc.encode(3.5), seed=1)
    c2 = orc.encrypt(pk, orc.encode(-2.25), seed=2)
    prod = np.stack([orc.multiply(c1, c2), orc.square(c1)])
    got = fhe.to_host(ev.relinearize(fhe.to_device(prod), evk_dev, dbc))
    for i in range(2):
        assert np.array_equal(got[i], orc.relinearize(prod[i], evk, dbc=dbc))
    # FHE_RELIN_FUSED=1: the key-switch sums formed inside the inverse-transform kernel (k_relin_accum_inv_add_pm) where the default runs
    # the accumulation and the inverse transform + addition as two launches (k_relin_accum_pm + k_relin_inv_add_pm): same bits;
    # and a batch that is not a multiple of anything, out of place (fhe_relinearize_to) with an operand at q - 1
    alt = _variant(fhe, ctx, FHE_RELIN_FUSED=1)
    big = np.concatenate([prod, prod[::-1], prod[:1]])
    for i, q in enumerate(ctx.q):
        big[4, :, i, :] = q - 1
    g1 = fhe.to_host(ev.relinearize(fhe.to_device(big), evk_dev, dbc))
    g2 = fhe.to_host(fhe.Evaluator(alt).relinearize(fhe.to_device(big), evk_dev, dbc))
    assert np.array_equal(g1, g2) and np.array_equal(g1[:2], got) and np.array_equal(g1[4], orc.relinearize(big[4], evk, dbc=dbc))
    assert orc.decode(orc.decrypt(sk, got[0])[0]) == 3.5 * -2.25
    assert orc.decode(orc.decrypt(sk, got[1])[0]) == 3.5 * 3.5


# ---------------------------------------------------------------------------------------------
# resize and decode circuits (BASELINE.json configs[2], configs[3] shapes at test sizes)
# ---------------------------------------------------------------------------------------------
def test_cubic_linear_vs_oracle(fhe, oracle_mod):
    """Cubic at level 1 (size 2 -> 4) and level 2 (size 4 -> 6), Linear 2 -> 3 -> 4, batched"""
    ctx, orc = _pair(fhe, oracle_mod, "SMALL")
    ev = fhe.Evaluator(ctx)
    pc = fhe.circuits.PlainCache(ctx)
    h = fhe.to_host
    A, B, C, D = (ctx.random_ct(2, size=2, seed=400 + i) for i in range(4))
    t = ctx.random_ct(2, size=2, seed=410)
    r1 = fhe.circuits.cubic(ev, pc, A, B, C, D, t)
    assert r1.shape[-3] == 4
    for i in range(2):
        assert np.array_equal(h(r1)[i], orc.cubic(h(A)[i], h(B)[i], h(C)[i], h(D)[i], h(t)[i]))
    A4, B4, C4, D4 = (ctx.random_ct(2, size=4, seed=420 + i) for i in range(4))
    r2 = fhe.circuits.cubic(ev, pc, A4, B4, C4, D4, t)
    assert r2.shape[-3] == 6
    for i in range(2):
        assert np.array_equal(h(r2)[i], orc.cubic(h(A4)[i], h(B4)[i], h(C4)[i], h(D4)[i], h(t)[i]))
    l1 = fhe.circuits.linear(ev, pc, A, B, t)
    l2 = fhe.circuits.linear(ev, pc, l1, l1, t)
    assert l1.shape[-3] == 3 and l2.shape[-3] == 4
    for i in range(2):
        o1 = orc.linear(h(A)[i], h(B)[i], h(t)[i])
        assert np.array_equal(h(l1)[i], o1)
        assert np.array_equal(h(l2)[i], orc.linear(o1, o1, h(t)[i]))


@pytest.mark.parametrize("preset", ["P8192", "SEAL23_4096"])
def test_cubic_fused_tail_vs_three_products_and_oracle(fhe, oracle_mod, preset):
    """Cubic on pseudo-Mersenne bases: the three products' floor / back conversion, their sum, encode(0.5) = x^-1 and + B in ONE
    launch (k_behz_floor3_combine_pm) against FHE_CUBIC_UNFUSED=1 (three complete products + k_cubic_combine_g) and the oracle,
    level 1 (size 2 -> 4) and level 2 (4 -> 6), a batch that is not a multiple of anything, operands at q - 1"""
    import torch
    ctx, orc = _pair(fhe, oracle_mod, preset)
    alt = _variant(fhe, ctx, FHE_CUBIC_UNFUSED=1)
    h = fhe.to_host
    t = ctx.random_ct(5, size=2, seed=410)
    for size in (2, 4):
        A, B, C, D = (ctx.random_ct(5, size=size, seed=400 + 10 * size + i) for i in range(4))
        A[1] = torch.tensor([q - 1 for q in ctx.q], dtype=torch.int64, device=A.device).view(1, ctx.k, 1).expand(size, ctx.k, ctx.n)
        got = fhe.circuits.cubic(fhe.Evaluator(ctx), fhe.circuits.PlainCache(ctx), A, B, C, D, t)
        want = fhe.circuits.cubic(fhe.Evaluator(alt), fhe.circuits.PlainCache(alt), A, B, C, D, t)
        assert got.shape[-3] == size + 2 and torch.equal(got, want)
        for i in (0, 1, 4):
            assert np.array_equal(h(got)[i], orc.cubic(h(A)[i], h(B)[i], h(C)[i], h(D)[i], h(t)[i])), (size, i)


def test_bicubic_resize_8x8_to_4x4(fhe, oracle_mod):
    """ResizeImage/SampleBicubic (homo/fhe_resize.h:254-392) on a small image, one channel:
    the product's batched sampler against per-pixel oracle Cubic calls, plus a decrypt known answer"""
    ctx, orc = _pair(fhe, oracle_mod, "SMALL")
    ev = fhe.Evaluator(ctx)
    pc = fhe.circuits.PlainCache(ctx)
    sk, pk = orc.keygen(21)
    W = H = 8
    w = h_ = 4
    vals = [float((29 * x + 53 * y) % 256) for y in range(H) for x in range(W)]
    pix = np.stack([orc.encrypt(pk, orc.encode(v), seed=500 + i) for i, v in enumerate(vals)])
    taps, fx, fy = fhe.circuits.resize_sample_plan(W, H, w, h_, bicubic=True)
    xf = np.stack([orc.encrypt(pk, orc.encode(f), seed=600 + i) for i, f in enumerate(fx)])
    yf = np.stack([orc.encrypt(pk, orc.encode(f), seed=700 + i) for i, f in enumerate(fy)])
    out = fhe.to_host(fhe.circuits.sample_bicubic(ev, pc, fhe.to_device(pix), taps, fhe.to_device(xf), fhe.to_device(yf)))
    assert out.shape == (w * h_, 6, ctx.k, ctx.n)

    def plain_cubic(A, B, C, D, t):     # closed form of homo/fhe_resize.h:149-185 with t3 = t*t
        a, b, c = -A + 3 * B - 3 * C + D, 2 * A - 5 * B + 4 * C - D, C - A
        return 0.5 * (a * t * t + b * t * t + c * t) + B

    for o in (0, 5, 15):
        p = [pix[i] for i in taps[o]]
        cols = [orc.cubic(p[4 * r], p[4 * r + 1], p[4 * r + 2], p[4 * r + 3], xf[o]) for r in range(4)]
        ref = orc.cubic(cols[0], cols[1], cols[2], cols[3], yf[o])
        assert np.array_equal(out[o], ref)
        v = [vals[i] for i in taps[o]]
        pc_cols = [plain_cubic(v[4 * r], v[4 * r + 1], v[4 * r + 2], v[4 * r + 3], fx[o]) for r in range(4)]
        expect = plain_cubic(pc_cols[0], pc_cols[1], pc_cols[2], pc_cols[3], fy[o])
        plain, budget = orc.decrypt(sk, out[o])
        assert budget > 0 and abs(orc.decode(plain) - expect) < 1e-6


def test_homomorphic_sin_cos_vs_oracle(fhe, oracle_mod):
    ctx, orc = _pair(fhe, oracle_mod, "SMALL")
    ev = fhe.Evaluator(ctx)
    pc = fhe.circuits.PlainCache(ctx)
    x, z = ctx.random_ct(2, size=2, seed=800), ctx.random_ct(2, size=2, seed=801)
    s = fhe.circuits.homomorphic_sin(ev, pc, x, z)
    c = fhe.circuits.homomorphic_cos(ev, pc, x, z)
    assert s.shape[-3] == 11 and c.shape[-3] == 11
    for i in range(2):
        assert np.array_equal(fhe.to_host(s)[i], oracle_mod.oracle_homomorphic_sin(orc, fhe.to_host(x)[i], fhe.to_host(z)[i]))
        assert np.array_equal(fhe.to_host(c)[i], oracle_mod.oracle_homomorphic_cos(orc, fhe.to_host(x)[i], fhe.to_host(z)[i]))


def test_approximated_step_vs_oracle(fhe, oracle_mod):
    """the deepest circuit (sizes up to 22) at a reduced size: W*H = 3 positions, 2 harmonics (unequal
    on purpose: the GPU path evaluates all position x harmonic pairs as one batch, the oracle serially)"""
    ctx, orc = _pair(fhe, oracle_mod, "SMALL")
    ev = fhe.Evaluator(ctx)
    pc = fhe.circuits.PlainCache(ctx)
    amp, idx, cnt = (ctx.random_ct(1, size=2, seed=900 + i) for i in range(3))
    zbank = {}

    def zeros_dev(i, j, which):
        return ctx.random_ct(1, size=2, seed=1000 + 100 * i + 10 * j + (which == "cos"))

    def zeros_host(i, j, which):
        return fhe.to_host(zeros_dev(i, j, which))[0]

    run = fhe.circuits.approximated_step(ev, pc, amp, idx, cnt, order=64, degree=2, delta=0.5, width=3, height=1, zeros=zeros_dev)
    ref = oracle_mod.oracle_approximated_step(orc, fhe.to_host(amp)[0], fhe.to_host(idx)[0], fhe.to_host(cnt)[0], 64, 2, 0.5, 3, 1, zeros_host)
    assert len(run) == 3
    for g, r in zip(run, ref):
        assert g.shape[-3] == 22
        assert np.array_equal(fhe.to_host(g)[0], r)


@pytest.mark.parametrize("preset", ["P8192", "SEAL23_4096"])
def test_plain_sums_with_one_inverse_transform_vs_separate_products(fhe, oracle_mod, preset):
    """the Taylor sums of homomorphic_sin / cos and the harmonic sum of approximated_step on pseudo-Mersenne bases: forward
    transform + slot product per term, ONE inverse transform per output polynomial (k_mulplain_fwd_pm + k_sum_inv_pm) against
    FHE_PLAIN_SUM_UNFUSED=1 (one multiply_plain per term, then the additions) -- the same bits -- and against the oracle"""
    import torch
    ctx, orc = _pair(fhe, oracle_mod, preset)
    alt = _variant(fhe, ctx, FHE_PLAIN_SUM_UNFUSED=1)
    x, z = ctx.random_ct(3, size=2, seed=810), ctx.random_ct(3, size=2, seed=811)
    x[1] = torch.tensor([q - 1 for q in ctx.q], dtype=torch.int64, device=x.device).view(1, ctx.k, 1).expand(2, ctx.k, ctx.n)
    outs = []
    for c in (ctx, alt):
        ev, pc = fhe.Evaluator(c), fhe.circuits.PlainCache(c)
        outs.append((fhe.circuits.homomorphic_sin(ev, pc, x, z), fhe.circuits.homomorphic_cos(ev, pc, x, z)))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert np.array_equal(fhe.to_host(outs[0][0])[1], oracle_mod.oracle_homomorphic_sin(orc, fhe.to_host(x)[1], fhe.to_host(z)[1]))
    assert np.array_equal(fhe.to_host(outs[0][1])[2], oracle_mod.oracle_homomorphic_cos(orc, fhe.to_host(x)[2], fhe.to_host(z)[2]))
    amp, idx, cnt = (ctx.random_ct(1, size=2, seed=910 + i) for i in range(3))
    zeros = ctx.random_ct(3 * 2 * 2, size=2, seed=920).reshape(3, 2, 2, 2, ctx.k, ctx.n)
    runs = [fhe.circuits.approximated_step(fhe.Evaluator(c), fhe.circuits.PlainCache(c), amp, idx, cnt, order=64, degree=2, delta=0.5, width=3, height=1,
                                           zeros=zeros) for c in (ctx, alt)]
    for g, w in zip(*runs):
        assert g.shape[-3] == 22 and torch.equal(g, w)
    hz = fhe.to_host(zeros)
    ref = oracle_mod.oracle_approximated_step(orc, fhe.to_host(amp)[0], fhe.to_host(idx)[0], fhe.to_host(cnt)[0], 64, 2, 0.5, 3, 1,
                                              lambda i, j, which: hz[i, j - 1, int(which == "cos")])
    assert np.array_equal(fhe.to_host(runs[0][2])[0], ref[2])


# ---------------------------------------------------------------------------------------------
# empty / ragged inputs and error behaviour of the C ABI
# ---------------------------------------------------------------------------------------------
def test_empty_inputs_are_no_ops(fhe, oracle_mod):
    import ctypes as C
    import torch
    ctx, _ = _pair(fhe, oracle_mod, "SMALL")
    L = fhe._lib.load()
    a = ctx.random_ct(1, seed=1)
    before = fhe.to_host(a).copy()
    p = C.c_void_p(a.data_ptr())
    assert L.fhe_add(ctx.h, p, p, p, 0, None) == 0
    assert L.fhe_negate(ctx.h, p, p, 0, None) == 0
    assert L.fhe_ntt_forward(ctx.h, p, p, 0, None) == 0
    assert L.fhe_multiply_plain(ctx.h, p, p, 0, p, None) == 0
    assert L.fhe_add_plain(ctx.h, p, 2 * ctx.k * ctx.n, 1, None, 0, 1, None) == 0     # zero plaintext
    plan = fhe.DctPlan(ctx, fhe.YQT)
    assert L.fhe_dct8x8_quant(ctx.h, plan.h, p, p, 0, None, 0, None) == 0
    assert L.fhe_fill_random(ctx.h, p, 0, 1, 0, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(fhe.to_host(a), before)


def test_ragged_block_counts(fhe, oracle_mod, monkeypatch):
    """block counts that do not divide the launch wave (7 blocks in waves of 3)"""
    ctx, orc = _pair(fhe, oracle_mod, "SMALL")
    ctx = _variant(fhe, ctx, FHE_DCT_WAVE_BLOCKS=3)
    ev = fhe.Evaluator(ctx)
    blocks = ctx.random_ct(7, 64, seed=77)
    out = fhe.to_host(ev.dct8x8_quant(fhe.DctPlan(ctx, fhe.YQT), blocks))
    for b in (0, 3, 6):
        assert np.array_equal(out[b], orc.dct_quant(fhe.to_host(blocks)[b], fhe.YQT))


def test_c_abi_error_codes(fhe, oracle_mod):
    import ctypes as C
    ctx, _ = _pair(fhe, oracle_mod, "SMALL")
    other = fhe.SEALContext(4096, oracle_mod.PRESETS["P4096"]["q"], 1 << 14)
    L = fhe._lib.load()
    a = ctx.random_ct(64, seed=1)
    p = C.c_void_p(a.data_ptr())
    plan_other = fhe.DctPlan(other, fhe.YQT)
    assert L.fhe_dct8x8_quant(ctx.h, plan_other.h, p, p, 1, None, 0, None) == -1        # plan of another context
    assert b"another context" in L.fhe_last_error()
    plan = fhe.DctPlan(ctx, fhe.YQT)
    assert L.fhe_dct8x8_quant(ctx.h, plan.h, p, p, 1, None, 0, None) == -1              # missing scratch
    assert b"scratch" in L.fhe_last_error()
    assert L.fhe_add(ctx.h, None, p, p, 1, None) == -1                                  # null pointer
    bad_plain = np.full(8, ctx.t, dtype=np.uint64)                                      # coefficient == t is out of range
    assert L.fhe_add_plain(ctx.h, p, 2 * ctx.k * ctx.n, 1, bad_plain.ctypes.data_as(C.c_void_p), 8, 1, None) == -1
    assert L.fhe_add_plain(ctx.h, p, 2 * ctx.k * ctx.n, 1, bad_plain.ctypes.data_as(C.c_void_p), 8, 0, None) == -1   # sign must be +-1
    assert L.fhe_multiply(ctx.h, p, 2, p, 2, p, 1, None, 0, None) == -1                 # scratch too small
    assert L.fhe_relinearize(ctx.h, p, 10, 1, p, 30, None, 0, None) == -1               # stride below a size-3 ciphertext
    # fhe_relinearize_to: the output either IS the input (same pointer and stride) or is disjoint from it -- a compacting in-place
    # call (3-polynomial inputs, 2-polynomial outputs at the same address) would let output c land on an input not yet read
    kn = ctx.k * ctx.n
    scr_bytes = L.fhe_relinearize_scratch_bytes(ctx.h, 30, 4)
    import torch
    scr = torch.empty(scr_bytes // 8 + 1, dtype=torch.int64, device=a.device)
    ps = C.c_void_p(scr.data_ptr())
    assert L.fhe_relinearize_to(ctx.h, p, 3 * kn, p, 2 * kn, 4, p, 30, ps, scr_bytes, None) == -1
    assert b"overlaps" in L.fhe_last_error()
    inside = C.c_void_p(a.data_ptr() + 8 * kn)
    assert L.fhe_relinearize_to(ctx.h, p, 3 * kn, inside, 3 * kn, 4, p, 30, ps, scr_bytes, None) == -1
    with pytest.raises(fhe.FheError):
        fhe._lib.call("fhe_ntt_forward", ctx.h, None, None, 1, None)
    h = C.c_void_p()
    q = (C.c_uint64 * 1)(0xFFFFEE001)
    assert L.fhe_ctx_create(4096, q, 1, 1 << 40, 0, C.byref(h)) == -1                   # t above the modulus
    q2 = (C.c_uint64 * 1)(0xFFFFEE003)
    assert L.fhe_ctx_create(4096, q2, 1, 1 << 14, 0, C.byref(h)) == -1                  # not an NTT prime
    assert L.fhe_ctx_create(4096, q, 1, 1 << 14, 99, C.byref(h)) == -1                  # no such device


# ---------------------------------------------------------------------------------------------
# the other polynomial degrees the reference's benchmark grid uses (benchmark/benchmark.py:6): 2048, 16384
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,q", [(2048, [0x3FFFFFFF000001]),
                                 (16384, [0x7FFFFFFF380001, 0x7FFFFFFEF00001, 0x3FFFFFFF000001])])
def test_other_degrees(fhe, oracle_mod, n, q):
    ctx, orc = fhe.SEALContext(n, q, 1 << 14), oracle_mod.Oracle(n, q, 1 << 14)
    ev, enc = fhe.Evaluator(ctx), fhe.FractionalEncoder(ctx)
    a, b = ctx.random_ct(2, seed=71), ctx.random_ct(2, seed=72)
    ha, hb = fhe.to_host(a), fhe.to_host(b)
    assert np.array_equal(fhe.to_host(ev.ntt_inverse(ev.ntt_forward(a))), ha)
    assert np.array_equal(fhe.to_host(ev.add(a, b))[1], orc.add(ha[1], hb[1]))
    for v in (0.541196100, -1.847759065, 3.0):
        assert np.array_equal(fhe.to_host(ev.multiply_plain(a, enc.encode(v)))[0], orc.multiply_plain(ha[0], orc.encode(v)))
    assert np.array_equal(fhe.to_host(ev.multiply(a, b))[0], orc.multiply(ha[0], hb[0]))
    blk = ctx.random_ct(1, 64, seed=73)
    out = fhe.to_host(ev.dct8x8_quant(fhe.DctPlan(ctx, fhe.YQT), blk))[0]
    ref = orc.dct_quant(fhe.to_host(blk)[0], fhe.YQT)
    assert np.array_equal(out, ref)


def test_ct_x_ct_with_seven_and_eight_coefficient_moduli(fhe, oracle_mod):
    """More than four coefficient moduli: the two-column sums of the base conversions run in two groups of columns per output
    (four y_i each), more than six: four groups of z_j -- shapes no preset reaches.  n = 2048, the largest 54-bit primes
    = 1 (mod 2^16); products and a square against the oracle."""
    primes, cand = [], (1 << 54) + 1 - (1 << 16)
    while len(primes) < 8:
        if _is_prime(cand):
            primes.append(cand)
        cand -= 1 << 16
    for k in (5, 7, 8):
        q = primes[:k]
        ctx, orc = fhe.SEALContext(2048, q, 1 << 14), oracle_mod.Oracle(2048, q, 1 << 14)
        assert fhe._lib.call("fhe_arith_path", ctx.h) == (1 | (2 << 2) | 16)
        ev = fhe.Evaluator(ctx)
        a, b = ctx.random_ct(3, seed=81), ctx.random_ct(3, seed=82)
        ha, hb = fhe.to_host(a), fhe.to_host(b)
        m = fhe.to_host(ev.multiply(a, b))
        for i in (0, 2):
            assert np.array_equal(m[i], orc.multiply(ha[i], hb[i])), (k, i)
        assert np.array_equal(fhe.to_host(ev.square(a))[1], orc.square(ha[1])), k


def _is_prime(m):
    if m < 2:
        return False
    for sp in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if m % sp == 0:
            return m == sp
    d, r = m - 1, 0
    while d % 2 == 0:
        d //= 2
        r += 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):      # deterministic below 3.3e24
        x = pow(a, d, m)
        if x in (1, m - 1):
            continue
        for _ in range(r - 1):
            x = x * x % m
            if x == m - 1:
                break
        else:
            return False
    return True


def _largest_ntt_prime_below(bits, n):
    c = (1 << bits) - 2 * n + 1
    while not _is_prime(c):
        c -= 2 * n
    assert c >> (bits - 1) == 1
    return c


@pytest.mark.parametrize("bits,n", [(56, 4096), (57, 4096), (58, 8192), (58, 16384), (59, 4096), (61, 8192)])
def test_u64_lazy_ranges_at_boundary_prime_sizes(fhe, oracle_mod, bits, n):
    """The u64 kernels choose their lazy ranges by prime size (csrc/ntt_core.h, csrc/dct_u64.hip): no conditional
    subtraction in the forward butterflies up to 58 bits (values grow to (2 + 4 log2 n) q, which must stay below 2^64),
    doubled Harvey ranges [0, 8q) above; the fused u64 DCT is lazy up to 56 bits and keeps one subtraction per
    butterfly at 57.  The LARGEST prime of each size with all-(q-1) inputs: the largest INPUTS the kernels take -- not the worst
    case of the lazy ranges (random data comes closer to the static bounds in almost every stage); the transforms at
    their arithmetic edges are in tests/test_gpu_ntt_extremes.py, the fused u64 DCT pair at 55, 56 and 57 bits and at all three n in
    tests/test_gpu_dct_u64_extremes.py."""
    q = [_largest_ntt_prime_below(bits, n), _largest_ntt_prime_below(bits - 1, n)]
    ctx, orc = fhe.SEALContext(n, q, 1 << 14), oracle_mod.Oracle(n, q, 1 << 14)
    ev = fhe.Evaluator(ctx)
    a = np.zeros((2, 2, ctx.k, ctx.n), dtype=np.uint64)
    for i, qi in enumerate(q):
        a[0, :, i, :] = qi - 1
    a[1] = fhe.to_host(ctx.random_ct(1, seed=91))[0]
    a[1, 0, :, ::3] = 0
    da = fhe.to_device(a)
    f = ev.ntt_forward(da)
    hf = fhe.to_host(f)
    for c in range(2):
        for i in range(ctx.k):
            assert np.array_equal(np.sort(hf[c, 1, i]), np.sort(orc.ntt_fwd(a[c, 1, i], i)))
    assert np.array_equal(fhe.to_host(ev.ntt_inverse(f)), a)
    rng = np.random.default_rng(17)
    plain = rng.integers(0, ctx.t, size=ctx.n, dtype=np.uint64)
    plain[:4] = ctx.t - 1
    got = fhe.to_host(ev.multiply_plain(da, plain))
    for c in range(2):
        assert np.array_equal(got[c], orc.multiply_plain(a[c], plain))
    prod = fhe.to_host(ev.multiply(da, da))
    for c in range(2):
        assert np.array_equal(prod[c], orc.multiply(a[c], a[c]))
    if n <= 8192:
        blk = np.zeros((1, 64, 2, ctx.k, ctx.n), dtype=np.uint64)
        for i, qi in enumerate(q):
            blk[0, :, :, i, :] = qi - 1
        blk[0, 7] = 0
        blk[0, 11, :, :, 1::2] = 1
        out = fhe.to_host(ev.dct8x8_quant(fhe.DctPlan(ctx, fhe.YQT), fhe.to_device(blk)))
        assert np.array_equal(out[0], orc.dct_quant(blk[0], fhe.YQT))


def test_plain_sums_on_a_58_bit_q_base(fhe, oracle_mod):
    """the PmB instantiation of k_mulplain_fwd_pm / k_sum_inv_pm (partial sums of eight terms below 1.5 q each on 58-bit primes):
    homomorphic_sin / cos on a q-base of the largest 58- and 57-bit NTT primes, an operand at q - 1, against the separate
    products and the oracle"""
    import torch
    n = 4096
    q = [_largest_ntt_prime_below(58, n), _largest_ntt_prime_below(57, n)]
    ctx, orc = fhe.SEALContext(n, q, 1 << 14), oracle_mod.Oracle(n, q, 1 << 14)
    assert fhe._lib.load().fhe_arith_path(ctx.h) & 3 == 2
    alt = _variant(fhe, ctx, FHE_PLAIN_SUM_UNFUSED=1)
    x, z = ctx.random_ct(2, size=2, seed=830), ctx.random_ct(2, size=2, seed=831)
    x[1] = torch.tensor([qi - 1 for qi in q], dtype=torch.int64, device=x.device).view(1, ctx.k, 1).expand(2, ctx.k, ctx.n)
    outs = []
    for c in (ctx, alt):
        ev, pc = fhe.Evaluator(c), fhe.circuits.PlainCache(c)
        outs.append((fhe.circuits.homomorphic_sin(ev, pc, x, z), fhe.circuits.homomorphic_cos(ev, pc, x, z)))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert np.array_equal(fhe.to_host(outs[0][0])[1], oracle_mod.oracle_homomorphic_sin(orc, fhe.to_host(x)[1], fhe.to_host(z)[1]))
    assert np.array_equal(fhe.to_host(outs[0][1])[0], oracle_mod.oracle_homomorphic_cos(orc, fhe.to_host(x)[0], fhe.to_host(z)[0]))


@pytest.mark.parametrize("bits,n", [(35, 8192), (34, 4096), (35, 16384)])
def test_u64_forward_canonicalisation_at_the_smallest_lazy_primes(fhe, oracle_mod, monkeypatch, bits, n):
    """canon_below_64q (csrc/ntt_core.h) estimates the quotient of the lazy forward transform's outputs from their high
    word in single precision; its error bound 2^32 / q is largest at the smallest primes the lazy kernels take (2^33):
    the u64 kernels forced onto 34- / 35-bit primes (the FP64 kernels would take them otherwise), all-(q-1) inputs"""
    q = [_largest_ntt_prime_below(bits, n), _largest_ntt_prime_below(bits - 1, n)]
    ctx, orc = fhe.SEALContext(n, q, 1 << 10, switches={"FHE_DCT_FORCE_U64": 1}), oracle_mod.Oracle(n, q, 1 << 10)
    ev = fhe.Evaluator(ctx)
    a = np.zeros((2, 2, ctx.k, ctx.n), dtype=np.uint64)
    for i, qi in enumerate(q):
        a[0, :, i, :] = qi - 1
    a[1] = fhe.to_host(ctx.random_ct(1, seed=92))[0]
    f = ev.ntt_forward(fhe.to_device(a))
    hf = fhe.to_host(f)
    for c in range(2):
        for i in range(ctx.k):
            assert hf[c, 1, i].max() < q[i]
            assert np.array_equal(np.sort(hf[c, 1, i]), np.sort(orc.ntt_fwd(a[c, 1, i], i)))
    assert np.array_equal(fhe.to_host(ev.ntt_inverse(f)), a)


@pytest.mark.parametrize("n_ct", [3, 4])
def test_fp64_transforms_and_multiply_plain_equal_u64_kernels(fhe, oracle_mod, monkeypatch, n_ct):
    """P4096: fhe_ntt_forward / fhe_ntt_inverse / fhe_multiply_plain on the FP64 kernels write the same
    words (same NTT-form order, canonical residues) as the u64 kernels; odd and even polynomial counts
    take the one- and two-polynomial workgroups.  multiply_plain also against the oracle."""
    import torch
    ctx, orc = _pair(fhe, oracle_mod, "P4096")
    ev = fhe.Evaluator(ctx)
    enc = fhe.FractionalEncoder(ctx)
    a = ctx.random_ct(n_ct, seed=5)
    if n_ct == 3:
        a = a.reshape(-1, ctx.k, ctx.n)[:5].contiguous()          # five RNS polynomials: odd count
    a.view(-1, ctx.k, ctx.n)[0] = torch.tensor([q - 1 for q in ctx.q], dtype=torch.int64, device=a.device).view(ctx.k, 1)
    plain = enc.encode(-0.168736)
    pp = fhe.PreparedPlain(ctx, plain)

    def run(e):
        f = e.ntt_forward(a)
        return f, e.ntt_inverse(f), (e.multiply_plain(a, pp) if n_ct == 4 else None)

    fast = run(ev)
    slow = run(fhe.Evaluator(_variant(fhe, ctx, FHE_DCT_FORCE_U64=1)))
    assert torch.equal(fast[0], slow[0]) and torch.equal(fast[1], slow[1]) and torch.equal(fast[1], a)
    if n_ct == 4:
        assert torch.equal(fast[2], slow[2])
        assert np.array_equal(fhe.to_host(fast[2])[1], orc.multiply_plain(fhe.to_host(a)[1], plain))


@pytest.mark.parametrize("preset", ["SMALL", "P4096", "P8192"])
def test_sparse_multiply_plain_equals_transform_path_and_oracle(fhe, oracle_mod, preset):
    """Plaintexts with few non-zero coefficients (the constants of Cubic: encode(3) = x+1, encode(5) =
    x^2+1, encode(4) = x^2, encode(0.5) = -x^(n-1), and -1) go through fhe_multiply_plain_sparse:
    same words as the NTT path and the oracle, also in place; dense plaintexts keep the NTT path."""
    import torch
    ctx, orc = _pair(fhe, oracle_mod, preset)
    ev = fhe.Evaluator(ctx)
    enc = fhe.FractionalEncoder(ctx)
    a = ctx.random_ct(3, seed=77)
    a[0, 0] = torch.tensor([q - 1 for q in ctx.q], dtype=torch.int64, device=a.device).view(ctx.k, 1)
    for v in (3.0, 5.0, 4.0, 2.0, 0.5, -1.0, 0.375):
        plain = enc.encode(v)
        pp = fhe.PreparedPlain(ctx, plain)
        assert pp.sparse
        got = ev.multiply_plain(a, pp)
        pp.sparse = False
        ref = ev.multiply_plain(a, pp)
        assert torch.equal(got, ref), v
        assert np.array_equal(fhe.to_host(got)[1], orc.multiply_plain(fhe.to_host(a)[1], plain)), v
        pp.sparse = True
        b = a.clone()
        ev.multiply_plain(b, pp, out=b)                      # in place
        assert torch.equal(b, ref), v
    assert not fhe.PreparedPlain(ctx, enc.encode(0.299)).sparse


@pytest.mark.parametrize("preset,size", [("SMALL", 2), ("P8192", 4)])
def test_fused_cubic_linear_parts_equal_evaluator_calls(fhe, oracle_mod, preset, size):
    """fhe_cubic (linear parts as single passes through index maps, t^2 formed once, prepared operands) against the
    same Cubic evaluated Evaluator call by Evaluator call (level 1: size-2 inputs; level 2: size-4 inputs, where
    c*t is one polynomial shorter than a*t3)."""
    import torch
    ctx, _ = _pair(fhe, oracle_mod, preset)
    ev = fhe.Evaluator(ctx)
    pc = fhe.circuits.PlainCache(ctx)
    A, B, C, D = (ctx.random_ct(3, size=size, seed=300 + i) for i in range(4))
    t = ctx.random_ct(3, size=2, seed=310)
    A[0, 0] = torch.tensor([q - 1 for q in ctx.q], dtype=torch.int64, device=A.device).view(ctx.k, 1)
    assert fhe.circuits._base2_cubic_constants(pc)
    fused = fhe.circuits.cubic(ev, pc, A, B, C, D, t)
    plain = fhe.circuits.cubic_evaluator_calls(ev, pc, A, B, C, D, t)
    assert fused.shape == plain.shape and fused.shape[-3] == size + 2
    assert torch.equal(fused, plain)


@pytest.mark.parametrize("preset", ["SMALL", "P4096"])
def test_multiply_with_prepared_operands(fhe, oracle_mod, preset):
    """fhe_multiply_prepared with either or both sides prepared equals fhe_multiply bit for bit
    (sizes 2x3 and 4x2), and a prepared operand can be reused."""
    import torch
    ctx, _ = _pair(fhe, oracle_mod, preset)
    ev = fhe.Evaluator(ctx)
    for sa, sb in ((2, 3), (4, 2)):
        a, b = ctx.random_ct(3, size=sa, seed=500 + sa), ctx.random_ct(3, size=sb, seed=600 + sb)
        ref = ev.multiply(a, b)
        pa, pb = ev.prepare_operand(a), ev.prepare_operand(b)
        assert torch.equal(ev.multiply(pa, b), ref)
        assert torch.equal(ev.multiply(a, pb), ref)
        assert torch.equal(ev.multiply(pa, pb), ref)
        a2 = ctx.random_ct(3, size=sa, seed=700 + sa)
        assert torch.equal(ev.multiply(a2, pb), ev.multiply(a2, b))


@pytest.mark.parametrize("preset", ["SMALL", "P4096", "P8192"])
def test_multiply_with_shared_prepared_operand(fhe, oracle_mod, preset):
    """fhe_multiply_prepared_shared: pair c multiplies entry (first + c // div) % count of a prepared batch; equal to
    fhe_multiply on the gathered operand bit for bit -- odd and even pair counts (the two-pair kernels at n = 8192
    and their one-pair remainder), both operand-side forms, wrap-around of the index."""
    import torch
    ctx, _ = _pair(fhe, oracle_mod, preset)
    ev = fhe.Evaluator(ctx)
    for sa, sb, count, nb, div, first in ((2, 3, 7, 3, 1, 0), (4, 3, 6, 4, 2, 1), (2, 2, 5, 2, 3, 5), (3, 2, 1, 4, 1, 2)):
        a, b = ctx.random_ct(count, size=sa, seed=510 + sa), ctx.random_ct(nb, size=sb, seed=610 + sb)
        idx = [(first + c // div) % nb for c in range(count)]
        ref = ev.multiply(a, b[torch.as_tensor(idx, device=b.device)].contiguous())
        pb = ev.prepare_operand(b)
        assert torch.equal(ev.multiply(a, pb.shared(div, first)), ref), (sa, sb, count)
        assert torch.equal(ev.multiply(ev.prepare_operand(a), pb.shared(div, first)), ref), (sa, sb, count)
        assert torch.equal(ev.multiply(a, pb.gather(idx)), ref), (sa, sb, count)


@pytest.mark.parametrize("preset", ["SMALL", "P4096", "SEAL23_4096"])
def test_randomised_op_sequences_vs_oracle(fhe, oracle_mod, preset):
    """seeded random sequences of Evaluator calls on small batches (odd and even counts, sparse and
    dense plaintexts, mixed sizes) replayed on the oracle: every intermediate must match bit for bit"""
    import random
    ctx, orc = _pair(fhe, oracle_mod, preset)
    ev = fhe.Evaluator(ctx)
    enc = fhe.FractionalEncoder(ctx)
    rng = random.Random(20260929 + len(preset))
    consts = [3.0, -2.0, 0.5, 0.299, -1.847759065, 128.0, 1.0 / 16, 0.587]
    for trial in range(6):
        count = rng.choice([1, 2, 3, 5])
        dev = [ctx.random_ct(count, size=2, seed=rng.randrange(1 << 30)) for _ in range(3)]
        host = [fhe.to_host(d).copy() for d in dev]            # [count, size, k, n]
        for step in range(5):
            op = rng.choice(["add", "sub", "negate", "mulplain", "addplain", "subplain", "multiply"])
            i, j = rng.randrange(3), rng.randrange(3)
            if op in ("add", "sub"):
                dev[i] = getattr(ev, op)(dev[i], dev[j])
                host[i] = np.stack([getattr(orc, op)(host[i][c], host[j][c]) for c in range(count)])
            elif op == "negate":
                dev[i] = ev.negate(dev[i])
                host[i] = np.stack([orc.negate(host[i][c]) for c in range(count)])
            elif op == "mulplain":
                p = enc.encode(rng.choice(consts))
                dev[i] = ev.multiply_plain(dev[i], p)
                host[i] = np.stack([orc.multiply_plain(host[i][c], p) for c in range(count)])
            elif op in ("addplain", "subplain"):
                p = enc.encode(rng.choice(consts))
                name = "add_plain" if op == "addplain" else "sub_plain"
                dev[i] = getattr(ev, name)(dev[i], p)
                host[i] = np.stack([getattr(orc, name)(host[i][c], p) for c in range(count)])
            else:
                if host[i].shape[1] + host[j].shape[1] > 5:
                    continue
                dev[i] = ev.multiply(dev[i], dev[j])
                host[i] = np.stack([orc.multiply(host[i][c], host[j][c]) for c in range(count)])
            assert np.array_equal(fhe.to_host(dev[i]), host[i]), (preset, trial, step, op)


# ---------------------------------------------------------------------------------------------
# the kernels behind the experiment switches (former defaults, fallbacks): same bits as the default path
# ---------------------------------------------------------------------------------------------
def test_presets_run_the_arithmetic_the_parity_tests_assume(fhe):
    """fhe_arith_path: the SEAL 2.3 presets (54/55-bit primes) take the pseudo-Mersenne kernels on both bases and the
    two-column base conversions, the 36/37-bit headline preset the Shoup / FP64 ones on its q-base and the pseudo-Mersenne
    ones on the 58-bit auxiliary base, and FHE_NTT_NOPM=1 switches all of it off -- so the parity tests above exercise the
    kernels their docstrings name."""
    path = lambda ctx: fhe._lib.call("fhe_arith_path", ctx.h)
    for preset in ("P8192", "SEAL23_4096", "SEAL23_2048"):
        assert path(fhe.SEALContext.preset(preset)) == (1 | (2 << 2) | 16), preset
    assert path(fhe.SEALContext.preset("P4096")) == (0 | (2 << 2) | 0)
    assert path(_variant(fhe, fhe.SEALContext.preset("P8192"), FHE_NTT_NOPM=1)) == 0
    assert path(_variant(fhe, fhe.SEALContext.preset("P8192"), FHE_BEHZ_AUX61=1)) == 1      # 61-bit auxiliary primes: Shoup kernels there, 128-bit conversions


@pytest.mark.parametrize("switch", ["FHE_NTT_NOPM", "FHE_BEHZ_AUX61", "FHE_BEHZ_CHUNK3", "FHE_NTT_NOPM+FHE_BEHZ_AUX61", "FHE_NTT_NOPM+FHE_BEHZ_CHUNK3",
                                    "FHE_NTT_NOPM+FHE_NTT_NOLAZY", "FHE_NTT_NOPM+FHE_NTT_SINGLE", "FHE_NTT_NOPM+FHE_BEHZ_TENSOR_CANON",
                                    "FHE_NTT_NOPM+FHE_BEHZ_TENSOR_SINGLE", "FHE_BEHZ_FUSED_PREPARE", "FHE_BEHZ_SQUARE_FULL"])
def test_fallback_kernels_give_the_same_bits(fhe, oracle_mod, switch):
    """Shoup butterflies where the pseudo-Mersenne ones run by default (FHE_NTT_NOPM), and under them the 61-bit
    auxiliary base, the three-term dot-product schedule, Harvey butterflies with conditional subtractions, one polynomial
    per workgroup, the canonical tensor sum; the 61-bit auxiliary base and the three-term schedule also beside the
    pseudo-Mersenne q-base kernels; FHE_BEHZ_FUSED_PREPARE: the base extension fused into the forward transforms (k_behz_prepare_pm) where the default runs it as its own launch (k_behz_to_bsk_pm + two transform
    launches); FHE_BEHZ_SQUARE_FULL: squares through the general tensor kernel (a_i a_j and a_j a_i both formed) where the default
    runs the symmetric instantiation (each cross term once, doubled).  Each is selected for a second context (the switches are read in fhe_ctx_create) and is
    bit-equal to the default kernels and to the oracle on transforms, multiply_plain and ct x ct products of sizes 2x2, 3x2
    and a square, at n = 8192 with 54/55-bit primes (where all of them differ from the default)."""
    import torch
    ctx, orc = _pair(fhe, oracle_mod, "P8192")
    alt = _variant(fhe, ctx, **{name: 1 for name in switch.split("+")})
    ev, ev2 = fhe.Evaluator(ctx), fhe.Evaluator(alt)
    a, b, c3 = ctx.random_ct(4, size=2, seed=41), ctx.random_ct(4, size=2, seed=42), ctx.random_ct(4, size=3, seed=43)
    a[0] = torch.tensor([q - 1 for q in ctx.q], dtype=torch.int64, device=a.device).view(1, ctx.k, 1).expand(2, ctx.k, ctx.n)
    pp, pp2 = (fhe.PreparedPlain(x, fhe.FractionalEncoder(x).encode(0.299)) for x in (ctx, alt))
    f = ev.ntt_forward(a)
    assert torch.equal(f, ev2.ntt_forward(a)) and torch.equal(ev2.ntt_inverse(f), a)
    assert torch.equal(ev.multiply_plain(a, pp), ev2.multiply_plain(a, pp2))
    m22, m32, sq = ev2.multiply(a, b), ev2.multiply(c3, b), ev2.square(c3)
    assert torch.equal(m22, ev.multiply(a, b)) and torch.equal(m32, ev.multiply(c3, b)) and torch.equal(sq, ev.square(c3))
    c5 = ctx.random_ct(3, size=5, seed=44)
    sq2, sq5 = ev.square(a), ev.square(c5)                        # even and odd numbers of cross terms, an operand at q - 1
    assert torch.equal(sq2, ev2.square(a)) and torch.equal(sq5, ev2.square(c5)) and torch.equal(sq2, ev.multiply(a, a.clone()))
    ha, hb = fhe.to_host(a), fhe.to_host(b)
    assert np.array_equal(fhe.to_host(m22)[0], orc.multiply(ha[0], hb[0]))
    assert np.array_equal(fhe.to_host(m22)[3], orc.multiply(ha[3], hb[3]))
    assert np.array_equal(fhe.to_host(sq2)[0], orc.multiply(ha[0], ha[0]))
    hc5 = fhe.to_host(c5)
    assert np.array_equal(fhe.to_host(sq5)[2], orc.multiply(hc5[2], hc5[2]))


@pytest.mark.parametrize("switches", [{"FHE_DCT_PIPELINE": 1, "FHE_DCT_WAVE_BLOCKS": 4}, {"FHE_DCT_PACK": 0}, {"FHE_DCT_LDSC": 0}, {"FHE_DCT_LE": 4}, {"FHE_DCT_ONE_LAUNCH": 2}])
def test_dct_variants_give_the_same_bits(fhe, oracle_mod, switches):
    """the two-stream pipelined mode (include/fhe_hip.h threading note), the FP64 intermediate, register-path constants,
    the 16-coefficient shape of the fused FP64 pair and the one-launch experiment (rows and columns in one grid, columns two
    units behind the rows, arrival counters) against the default launch and the oracle (P4096, 10 blocks:
    ragged against the 2-block half waves of the pipelined mode)"""
    ctx, orc = _pair(fhe, oracle_mod, "P4096")
    alt = _variant(fhe, ctx, **switches)
    blocks = ctx.random_ct(10, 64, seed=123)
    want = fhe.to_host(fhe.Evaluator(ctx).dct8x8_quant(fhe.DctPlan(ctx, fhe.YQT), blocks))
    got = fhe.to_host(fhe.Evaluator(alt).dct8x8_quant(fhe.DctPlan(alt, fhe.YQT), blocks))
    assert np.array_equal(got, want)
    assert np.array_equal(got[9], orc.dct_quant(fhe.to_host(blocks)[9], fhe.YQT))


def test_u64_fused_switch_selects_the_general_path(fhe, oracle_mod):
    ctx, orc = _pair(fhe, oracle_mod, "SEAL23_4096")
    alt = _variant(fhe, ctx, FHE_DCT_U64_FUSED=0)
    blocks = ctx.random_ct(3, 64, seed=5)
    want = fhe.to_host(fhe.Evaluator(ctx).dct8x8_quant(fhe.DctPlan(ctx, fhe.YQT), blocks))
    assert np.array_equal(fhe.to_host(fhe.Evaluator(alt).dct8x8_quant(fhe.DctPlan(alt, fhe.YQT), blocks)), want)
    assert np.array_equal(want[1], orc.dct_quant(fhe.to_host(blocks)[1], fhe.YQT))


@pytest.mark.parametrize("preset", ["SMALL", "P8192"])
def test_add_sub_of_unequal_sizes_batched(fhe, oracle_mod, preset):
    """fhe_add_sizes: seal::Evaluator::add / sub where the destination grows (homo/fhe_resize.h:181-184, homo/fhe_decode.h:114-118,237),
    for a whole batch in one launch -- against the oracle's fo_add / fo_sub and the golden big-integer vectors' conventions
    (missing polynomials count as zero; a - b negates the tail of b); out aliasing the longer operand"""
    import ctypes as C
    import torch
    ctx, orc = _pair(fhe, oracle_mod, preset)
    L = fhe._lib
    for sa, sb in ((2, 4), (4, 2), (3, 2), (2, 5), (1, 3)):
        a, b = ctx.random_ct(5, size=sa, seed=60 + sa), ctx.random_ct(5, size=sb, seed=70 + sb)
        a[1] = torch.tensor([q - 1 for q in ctx.q], dtype=torch.int64, device=a.device).view(1, ctx.k, 1).expand(sa, ctx.k, ctx.n)
        ha, hb = fhe.to_host(a), fhe.to_host(b)
        for sub in (0, 1):
            out = ctx.empty(5, size=max(sa, sb))
            L.call("fhe_add_sizes", ctx.h, C.c_void_p(a.data_ptr()), sa, C.c_void_p(b.data_ptr()), sb, C.c_void_p(out.data_ptr()), 5, sub, None)
            got = fhe.to_host(out)
            for i in (0, 1, 4):
                assert np.array_equal(got[i], (orc.sub if sub else orc.add)(ha[i], hb[i])), (sa, sb, sub, i)
        big, small, s_big = (a, b, sa) if sa > sb else (b, a, sb)
        alias = big.clone()                                                      # in place on the longer operand
        L.call("fhe_add_sizes", ctx.h, C.c_void_p(alias.data_ptr()), s_big, C.c_void_p(small.data_ptr()), min(sa, sb), C.c_void_p(alias.data_ptr()), 5, 0, None)
        assert np.array_equal(fhe.to_host(alias)[2], orc.add(fhe.to_host(big)[2], fhe.to_host(small)[2]))
    with pytest.raises(fhe._lib.FheError):
        L.call("fhe_add_sizes", ctx.h, C.c_void_p(a.data_ptr()), 0, C.c_void_p(b.data_ptr()), 2, C.c_void_p(a.data_ptr()), 1, 0, None)


def test_add_sub_refuse_operands_of_different_counts(fhe):
    """Evaluator.add / sub hand the library two pointers and ONE count: operands that are not the same number of ciphertexts of this context,
    or an `out` of another size, are an error in the host -- not a read or write behind the shorter tensor"""
    import torch
    ctx = fhe.SEALContext.preset("SEAL23_2048")
    ev = fhe.Evaluator(ctx)
    a, b = ctx.random_ct(4, size=2, seed=1), ctx.random_ct(3, size=2, seed=2)
    for op in (ev.add, ev.sub):
        with pytest.raises(ValueError, match="same number of ciphertexts"):
            op(a, b)
        with pytest.raises(ValueError, match="same number of ciphertexts"):
            op(a, ctx.random_ct(3, size=3, seed=2))
        with pytest.raises(ValueError, match="same number of ciphertexts"):
            op(a, a[..., : ctx.n // 2].contiguous())
        with pytest.raises(ValueError, match="out"):
            op(a, a, out=torch.empty_like(b))
    one = ctx.random_ct(1, size=2, seed=3)
    assert torch.equal(ev.add(one, one[0]), ev.add(one, one))              # [1, 2, k, n] with [2, k, n]: the same single ciphertext
    assert ev.add(a, ctx.random_ct(4, size=3, seed=5)).shape[-3] == 3


def test_fused_ops_refuse_mismatched_tensors(fhe):
    """dct8x8_quant with an `out` of another shape, rgb_to_ycc with channels of different counts: refused by the host (one count goes to the library)"""
    import torch
    ctx = fhe.SEALContext.preset("SEAL23_2048")
    ev = fhe.Evaluator(ctx)
    blocks = ctx.random_ct(2, 64, seed=1)
    plan = fhe.DctPlan(ctx, fhe.YQT)
    with pytest.raises(ValueError, match="out"):
        ev.dct8x8_quant(plan, blocks, out=torch.empty_like(blocks[:1]))
    r, g, b = ctx.random_ct(4, seed=1), ctx.random_ct(4, seed=2), ctx.random_ct(3, seed=3)
    with pytest.raises(ValueError, match="one shape"):
        ev.rgb_to_ycc(r, g, b)
    with pytest.raises(ValueError, match="one shape"):
        ev.rgb_to_ycc(r, g, ctx.random_ct(4, size=3, seed=3))
    ev.rgb_to_ycc(r, g, ctx.random_ct(4, seed=3))
    assert ev.dct8x8_quant(plan, blocks, out=torch.empty_like(blocks)).shape == blocks.shape


def test_empty_batches_through_the_python_host_are_no_ops(fhe):
    """An empty torch tensor has no storage (data_ptr() == 0) and the C ABI refuses null pointers before it looks at the count: the host hands
    the library a placeholder address for empty tensors (evaluator._ptr), so a rank whose shard of a small image is empty, a channel without runs or
    a zero-pixel band goes through every entry point as the no-op the C ABI defines for count == 0 -- with outputs of the right (empty) shape."""
    import torch
    ctx = fhe.SEALContext.preset("SEAL23_4096")
    ev, pc = fhe.Evaluator(ctx), fhe.circuits.PlainCache(ctx)
    kg = fhe.KeyGenerator(ctx, seed=1)
    evk = kg.generate_evaluation_keys(30, 2).contiguous()
    e2, e3, e4 = ctx.empty(0), ctx.empty(0, size=3), ctx.empty(0, size=4)
    k, n = ctx.k, ctx.n
    assert ev.add(e2, e2).shape == ev.sub(e2, e2).shape == ev.negate(e2).shape == (0, 2, k, n)
    assert ev.multiply(e2, e2).shape == ev.square(e2).shape == (0, 3, k, n)
    assert ev.multiply(e3, e2).shape == (0, 4, k, n)
    assert ev.relinearize(e3, evk, 30).shape == ev.relinearize(e4, evk, 30).shape == (0, 2, k, n)
    assert ev.multiply_plain(e2, pc.prepared(0.5)).shape == ev.add_plain(e2, pc.plain(3.0)).shape == (0, 2, k, n)
    assert ev.rgb_to_ycc(ctx.empty(0), ctx.empty(0), ctx.empty(0))[0].shape == (0, 2, k, n)
    assert ev.ntt_inverse(ev.ntt_forward(e2)).shape == (0, 2, k, n)
    assert ev.dct8x8_quant(fhe.DctPlan(ctx, fhe.YQT), ctx.empty(0, 64)).shape == (0, 64, 2, k, n)
    assert ctx.digest(e2.view(-1)) == 0
    for relin in (None, (evk, 30), (evk, 30, "cubic")):
        want = 2 if relin else 4
        assert fhe.circuits.cubic(ev, pc, e2, e2, e2, e2, e2, relin=relin).shape == (0, want, k, n)
        assert fhe.circuits.linear(ev, pc, e2, e2, e2, relin=relin).shape == (0, 2 if relin else 3, k, n)
    pix = ctx.random_ct(16, seed=1)
    taps, _, _ = fhe.circuits.resize_sample_plan(4, 4, 2, 2, bicubic=True)
    assert fhe.circuits.sample_bicubic(ev, pc, pix, taps[:0], e2, e2).shape == (0, 6, k, n)
    assert fhe.circuits.homomorphic_sin(ev, pc, e2, e2).shape == (0, 11, k, n)
    der, dec = fhe.DeviceEncryptor(ctx, kg.public_key()), fhe.Decryptor(ctx, kg.secret_key())
    assert der.encrypt_values(np.zeros(0)).shape == der.encrypt_zeros(0).shape == (0, 2, k, n)
    assert dec.decrypt_batch(e2).shape == (0, n)
    torch.cuda.synchronize()
    # and a shard loop in which one rank owns nothing: three blocks over a world of four
    plan, blocks = fhe.DctPlan(ctx, fhe.YQT), ctx.random_ct(3, 64, seed=5)
    whole = ev.dct8x8_quant(plan, blocks)
    parts = [ev.dct8x8_quant(plan, blocks[s:e].contiguous()) for s, e in (fhe.parallel.block_range(r, 4, 3) for r in range(4))]
    assert parts[3].shape[0] == 0 and torch.equal(torch.cat(parts), whole)


def test_buffers_beyond_2_to_the_32_words(fhe, oracle_mod):
    """Maximum sizes: 288 GB of HBM holds batches whose WORD offsets pass 2^32 (3,072 blocks of the headline configuration = 4.8e9 words, 39 GB in and
    39 GB out).  The fused DCT pair on the whole batch equals the oracle on blocks either side of the 2^31 / 2^32 word boundaries and at the end, equals
    itself evaluated in three 1,024-block pieces, the position-keyed digest of the whole equals the sum over the pieces, and add / NTT round trips over
    the same 196,608 ciphertexts are exact at the far end -- a 32-bit index anywhere in a kernel would show here."""
    import torch
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < 100 * 2 ** 30:
        pytest.skip("needs 100 GB of free HBM")
    om = oracle_mod
    ctx = fhe.SEALContext.preset("P4096")
    ev, plan, orc = fhe.Evaluator(ctx), fhe.DctPlan(ctx, fhe.YQT), om.Oracle.preset("P4096")
    B, wpb = 3072, 64 * 2 * ctx.k * ctx.n
    assert B * wpb > 2 ** 32
    blocks = ctx.random_ct(B, 64, seed=fhe.SEED)
    out = ev.dct8x8_quant(plan, blocks)
    for b in (1365, 2730, 2731, B - 1):                       # word offsets 2^31 - 5e5, 2^32 - 1e6, 2^32 + 5e5, 4.83e9
        assert np.array_equal(fhe.to_host(out[b]), orc.dct_quant(fhe.to_host(blocks[b]), om.YQT)), b
    piece = torch.empty_like(blocks[:1024])
    parts = 0
    for c in range(3):
        ev.dct8x8_quant(plan, blocks[c * 1024:(c + 1) * 1024], out=piece)
        assert torch.equal(piece, out[c * 1024:(c + 1) * 1024])
        parts += ctx.digest(piece.view(-1), index0=c * 1024 * wpb)
    assert ctx.digest(out.view(-1)) == parts % (1 << 64)
    del piece
    a, o = blocks.view(-1, 2, ctx.k, ctx.n), out.view(-1, 2, ctx.k, ctx.n)
    last = a.shape[0] - 1
    ev.add(a, a, out=o)
    ha = fhe.to_host(a[last])
    want = np.stack([[(ha[j, i].astype(object) * 2 % int(ctx.q[i])).astype(np.uint64) for i in range(ctx.k)] for j in range(2)])
    assert np.array_equal(fhe.to_host(o[last]), want)
    ev.ntt_forward(a, out=o)
    ev.ntt_inverse(o, out=o)
    assert torch.equal(o, a)
    del blocks, out, a, o
    torch.cuda.empty_cache()


def test_ctct_scratch_beyond_2_to_the_32_words(fhe):
    """The same for the BEHZ pipeline: 9,216 products at n = 8192 take 35 GB of scratch (4.7e9 words); multiply, square and a relinearize of the
    products equal the same calls on 1,024-ciphertext pieces, bit for bit (the pieces' scratch stays far below 2^31 words)."""
    import torch
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < 100 * 2 ** 30:
        pytest.skip("needs 100 GB of free HBM")
    ctx = fhe.SEALContext.preset("P8192")
    ev, L, N = fhe.Evaluator(ctx), fhe._lib.load(), 9216
    assert L.fhe_multiply_scratch_bytes(ctx.h, 2, 2, N) // 8 > 2 ** 32
    a, b = ctx.random_ct(N, seed=1), ctx.random_ct(N, seed=2)
    whole, sq = ev.multiply(a, b), ev.square(a)
    evk = fhe.KeyGenerator(ctx, seed=3).generate_evaluation_keys(30, 1).contiguous()
    rel = ev.relinearize(whole, evk, 30)
    small = fhe.Evaluator(ctx)                                 # its own (small) scratch buffer
    for c in range(N // 1024):
        s = slice(c * 1024, (c + 1) * 1024)
        pa, pb = a[s].contiguous(), b[s].contiguous()
        assert torch.equal(small.multiply(pa, pb), whole[s]) and torch.equal(small.square(pa), sq[s])
        assert torch.equal(small.relinearize(whole[s].contiguous(), evk, 30), rel[s])
    del whole, sq, rel, a, b
    ev._scratch = None
    torch.cuda.empty_cache()


def test_cubic_scratch_beyond_2_to_the_32_words(fhe):
    """... and for the batched circuits: 4,096 Cubics at n = 8192 take 46 GB of scratch (6.2e9 words); equal to four 1,024-tuple pieces, bit for bit"""
    import torch
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < 100 * 2 ** 30:
        pytest.skip("needs 100 GB of free HBM")
    ctx = fhe.SEALContext.preset("P8192")
    ev, pc, K, M = fhe.Evaluator(ctx), fhe.circuits.PlainCache(ctx), fhe.circuits, 4096
    assert fhe._lib.load().fhe_cubic_scratch_bytes(K.circuits_of(pc).h, 2, M) // 8 > 2 ** 32
    ops = [ctx.random_ct(M, seed=10 + i) for i in range(5)]
    whole = K.cubic(ev, pc, *ops)
    K.circuits_of(pc)._scratch = None
    torch.cuda.empty_cache()
    for c in range(M // 1024):
        s = slice(c * 1024, (c + 1) * 1024)
        assert torch.equal(K.cubic(ev, pc, *[o[s].contiguous() for o in ops]), whole[s])
    K.circuits_of(pc)._scratch = None
    del whole, ops
    torch.cuda.empty_cache()


@pytest.mark.parametrize("preset,B,P,path", [("SEAL23_4096", 4224, 1056, 2), ("P8192", 1100, 275, 2), ("SEAL23_16384", 288, 96, 0)])
def test_other_dct_paths_beyond_2_to_the_32_words(fhe, preset, B, P, path):
    """the u64 fused pair (SEAL 2.3.1's 54 / 55-bit primes at n = 4096 and 8192) and the general three-launch path (n = 16384) on batches of more than
    2^32 words: equal to the same call on quarter-size pieces, digests add up"""
    import torch
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < 100 * 2 ** 30:
        pytest.skip("needs 100 GB of free HBM")
    ctx = fhe.SEALContext.preset(preset)
    ev, plan = fhe.Evaluator(ctx), fhe.DctPlan(ctx, fhe.YQT)
    wpb = 64 * 2 * ctx.k * ctx.n
    assert B * wpb > 2 ** 32 and fhe._lib.load().fhe_dct_path(ctx.h) == path
    blocks = ctx.random_ct(B, 64, seed=fhe.SEED)
    out = ev.dct8x8_quant(plan, blocks)
    piece, parts = torch.empty_like(blocks[:P]), 0
    for c in range(B // P):
        ev.dct8x8_quant(plan, blocks[c * P:(c + 1) * P], out=piece)
        assert torch.equal(piece, out[c * P:(c + 1) * P]), c
        parts += ctx.digest(piece.view(-1), index0=c * P * wpb)
    assert ctx.digest(out.view(-1)) == parts % (1 << 64)
    del blocks, out, piece
    ev._scratch = None
    torch.cuda.empty_cache()
