"""CPU: the specification of the integer linear maps across slot-packed ciphertexts holds on the unchanged oracle in both of its forms
(tests/packed_oracle.py); the host-only pieces -- fhe_dct8_matrix, the fixed-point JPEG plans and their bound, pack_blocks / unpack_blocks /
descale -- against numpy; and the checks of the new entry points that need no device."""
import ctypes as C
import os

import numpy as np
import pytest

import galois_oracle as go
import packed_oracle as po

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boazbarak_stb_rgb.npy")


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("size", [2, 3])
def test_the_two_forms_of_the_specification_agree(oracle_mod, size):
    """op-by-op on the oracle == direct evaluation modulo q_i, n = 64, random residues: block map (with and without pre / post) and channel mix"""
    n, t = 64, po.T33
    for q in (go.Q3, go.Q4):
        orc = oracle_mod.Oracle(n, q, t)
        rng = np.random.default_rng(size + len(q))
        X = orc.random_ct(64, size=size, seed=11 + size)
        X[3] = np.array(q, dtype=np.uint64)[None, :, None] - np.uint64(1)          # one ciphertext of q_i - 1
        for pre, post in ((True, True), (False, False)):
            L, R, p0, p1 = po.random_plan(rng, t, pre, post)
            want = po.block8x8_compose(orc, X, L, R, p0, p1)
            assert np.array_equal(po.block8x8_direct(q, X, L, R, p0, p1), want), (len(q), size, pre, post)
        lim = po.scalar_limit(t)
        for c, m in ((1, 1), (3, 3), (8, 2)):
            M = rng.integers(-lim, lim + 1, size=(m, c), dtype=np.int64)
            M[0, 0] = lim
            if c > 1:
                M[m - 1, 1] = 0
            bias = rng.integers(-lim, lim + 1, size=m, dtype=np.int64)
            bias[0] = -lim
            planes = X[:c]
            for b in (None, bias):
                want = po.channel_mix_compose(orc, M, planes, b)
                assert np.array_equal(po.channel_mix_direct(q, t, M, planes, b), want), (len(q), size, c, m, b is None)


def test_composition_decrypts_to_the_integer_matrix_product(oracle_mod):
    """real oracle encryptions of batch-encoded slots, t = 65537, n = 64: the composition decrypts, in every slot, to
    post * (L (pre * X) R^T) modulo t, and the channel mix to M x + bias"""
    n, t = 64, go.T_BATCH
    orc = oracle_mod.Oracle(n, go.Q3, t)
    sk, pk = orc.keygen(seed=5)
    rng = np.random.default_rng(1)
    slots = rng.integers(0, t, size=(64, n), dtype=np.uint64)
    cts = np.stack([orc.encrypt(pk, go.encode_slots(slots[p], n, t), seed=100 + p) for p in range(64)])
    L, R, pre, post = (rng.integers(-9, 10, size=(8, 8)) for _ in range(4))
    L[(np.abs(L).sum(axis=1) == 0), 0] = 1
    R[(np.abs(R).sum(axis=1) == 0), 0] = 1
    pre[pre == 0], post[post == 0] = 1, -1
    out = po.block8x8_compose(orc, cts, L, R, pre, post)
    x = slots.astype(object).reshape(8, 8, n)
    want = np.einsum("ux,xyn,vy->uvn", L.astype(object), x * pre.astype(object)[:, :, None], R.astype(object)) * post.astype(object)[:, :, None]
    budgets = []
    for p in range(64):
        plain, budget = orc.decrypt(sk, out[p])
        budgets.append(budget)
        assert np.array_equal(go.decode_slots(plain, n, t), (want[p // 8, p % 8] % t).astype(np.uint64)), p
    print("\n[packed oracle n=%d] noise budget left %d bits" % (n, min(budgets)))
    assert min(budgets) > 0
    M, bias = np.array([[77, 150, 29], [-43, -85, 128], [128, -107, -21]]), [-32768, 0, 5]
    mixed = po.channel_mix_compose(orc, M, cts[:3], bias)
    for i in range(3):
        plain, budget = orc.decrypt(sk, mixed[i])
        want_i = (sum(int(M[i][j]) * slots[j].astype(object) for j in range(3)) + bias[i]) % t
        assert budget > 0 and np.array_equal(go.decode_slots(plain, n, t), want_i.astype(np.uint64)), i


def test_dct8_matrix(fhe):
    lib = fhe._lib.load()
    D = np.zeros(64, dtype=np.int64)
    assert lib.fhe_dct8_matrix(8, _vp(D)) == 0
    assert list(D[:8]) == [91] * 8 and list(D[8:16]) == [126, 106, 71, 25, -25, -71, -106, -126]
    assert lib.fhe_dct8_matrix(10, _vp(D)) == 0
    assert list(D[:8]) == [362] * 8 and list(D[8:16]) == [502, 426, 284, 100, -100, -284, -426, -502]
    u, x = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    for bits in range(1, 21):
        assert lib.fhe_dct8_matrix(bits, _vp(D)) == 0
        M = D.reshape(8, 8)
        for r in range(8):
            assert np.array_equal(M[r, ::-1], M[r] * (-1) ** r), (bits, r)          # row u is (-1)^u-symmetric
        exact = np.where(u == 0, np.sqrt(0.5), 1.0) * 0.5 * np.cos((2 * x + 1) * u * np.pi / 16) * 2.0 ** bits
        assert np.abs(M - exact).max() <= 0.5 + 1e-6
        assert np.array_equal(fhe.circuits.dct8_matrix(bits), M)
    for bits in (0, 21, -1):
        assert lib.fhe_dct8_matrix(bits, _vp(D)) == -1 and b"dct8_matrix" in lib.fhe_last_error()
    assert lib.fhe_dct8_matrix(8, None) == -1


def _golden_channels():
    rgb = np.load(GOLDEN)
    assert rgb.shape == (48, 48, 3)
    return [rgb[:, :, c].astype(np.int64) - 128 for c in range(3)]


def check_against_float(got, channels, quant):
    """the issue's condition: every coefficient within 1 of round-half-away(float64 DCT / Q), at most 2 % of them different"""
    diff = total = worst = 0
    for ch, g in zip(channels, got):
        ref = po.float_dct_quant(po.blocks8(ch), quant)
        d = np.abs(np.asarray(g).astype(np.int64) - ref)
        worst, diff, total = max(worst, int(d.max())), diff + int((d != 0).sum()), total + d.size
    print("\n[packed dct vs float64] %d of %d coefficients differ (%.2f %%), max |diff| %d" % (diff, total, 100.0 * diff / total, worst))
    assert total == 6912 and worst <= 1 and diff <= 0.02 * total
    return diff


def test_plan_builders_on_the_golden_image(fhe):
    """the exact integer model of packed_dct_plan at the defaults (8, 8) on 48 x 48 x 3 level-shifted pixels (36 blocks per channel)"""
    circuits, client = fhe.circuits, fhe.client
    plan = circuits.packed_dct_plan(None)
    D = circuits.dct8_matrix(8)
    Q = np.array(fhe.YQT).reshape(8, 8)
    assert plan.scale_bits == 24 and np.array_equal(plan.L, D) and np.array_equal(plan.R, D) and plan.pre is None
    assert np.array_equal(plan.post, (512 + Q) // (2 * Q))
    channels = _golden_channels()
    got = []
    for ch in channels:
        y = plan.model(po.blocks8(ch))
        assert int(np.abs(y).max()) <= plan.bound(128)
        got.append(client.descale(y % po.T33, plan.scale_bits, po.T33))
    assert check_against_float(got, channels, Q) == 92
    # the inverse plan: pre = Q (exact dequantisation), the transposes, and pixels back within the bound the model itself gives
    inv = circuits.packed_idct_plan(None)
    assert inv.scale_bits == 16 and np.array_equal(inv.pre, Q) and np.array_equal(inv.L, D.T) and np.array_equal(inv.R, D.T) and inv.post is None
    back = client.descale(inv.model(got[0]) % po.T33, inv.scale_bits, po.T33)
    assert int(np.abs(inv.model(got[0])).max()) <= inv.bound(np.abs(got[0]).max(axis=0)) < po.T33 // 2
    print("[packed idct] max pixel error after quantisation %d" % int(np.abs(back - po.blocks8(channels[0])).max()))


def test_forward_bound(fhe):
    plan = fhe.circuits.packed_dct_plan(None)
    assert plan.bound(128) == 1618419712
    assert po.T33 == 0x100050001 and go.is_prime(po.T33) and po.T33 % 32768 == 1
    assert plan.bound(128) < po.T33 // 2
    assert plan.bound(np.full((8, 8), 128)) == plan.bound(128)
    M = fhe.circuits.packed_rgb_to_ycc(8)
    assert M.tolist() == [[77, 150, 29], [-43, -85, 128], [128, -107, -21]]
    assert fhe.circuits.packed_ycc_to_rgb(8).tolist() == [[256, 0, 359], [256, -88, -183], [256, 454, 0]]
    # behind the colour mix (|value| <= 128 * 2^8 after the level shift) the forward plan needs the 41-bit modulus
    assert go.is_prime(po.T41) and po.T41 % 32768 == 1 and plan.bound(128 << 8) < po.T41 // 2


def test_pack_blocks_round_trip(fhe):
    client = fhe.client
    rng = np.random.default_rng(4)
    for (w, h, n) in ((48, 48, 16), (48, 48, 64), (40, 24, 4), (8, 8, 4)):         # 36 blocks in groups of 16: not a multiple
        ch = rng.integers(-128, 128, size=(h, w))
        s = client.pack_blocks(ch, w, h, n)
        blocks = client.blocks_of(ch, w, h)
        assert s.shape == ((len(blocks) + n - 1) // n, 64, n)
        for b, blk in enumerate(blocks):
            assert np.array_equal(s[b // n, :, b % n], blk)
        used = np.zeros(s.shape[0] * n, dtype=bool)
        used[:len(blocks)] = True
        assert not s.transpose(0, 2, 1).reshape(-1, 64)[~used].any()               # unused slots are 0
        assert np.array_equal(client.unpack_blocks(s, w, h), ch)
        sm = client.pack_blocks(ch, w, h, n, t=po.T33)
        assert sm.dtype == np.uint64 and np.array_equal(client.descale(sm, 0, po.T33), s)
    v = np.array([0, 383, 384, 385, po.T33 - 383, po.T33 - 384, po.T33 - 1, (po.T33 - 1) // 2, (po.T33 + 1) // 2], dtype=np.uint64)
    assert client.descale(v, 8, po.T33).tolist() == [0, 1, 2, 2, -1, -2, 0, ((po.T33 - 1) // 2 + 128) >> 8, -(((po.T33 - 1) // 2 + 128) >> 8)]


def test_new_entry_points_refuse_null_arguments(fhe):
    """the checks that need no device: a null context or operand is FHE_ERR_PARAM"""
    lib = fhe._lib.load()
    buf = np.zeros(64, dtype=np.int64)
    h = C.c_void_p()
    assert lib.fhe_block8x8_plan_create(None, _vp(buf), _vp(buf), None, None, None, C.byref(h)) == -1 and b"null argument" in lib.fhe_last_error()
    assert not h.value
    assert lib.fhe_block8x8_plan_destroy(None) == 0
    assert lib.fhe_block8x8_scalar(None, None, _vp(buf), _vp(buf), 2, 1, None) == -1 and b"null argument" in lib.fhe_last_error()
    assert lib.fhe_channel_mix(None, _vp(buf), None, 3, 3, _vp(buf), 8, 8, _vp(buf), 8, 8, 2, 1, None) == -1 and b"null argument" in lib.fhe_last_error()
