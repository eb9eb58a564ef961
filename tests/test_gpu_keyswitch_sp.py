"""GPU: the key switch with a special prime (include/fhe_hip.h fhe_relinearize_sp_poly / fhe_apply_galois_sp; csrc/keyswitch_sp.hip) against
its specification on the unchanged CPU oracle (tests/keyswitch_sp_oracle.py), bit for bit: random operands and the crafted families R
(reduction edges), D (drop edges) and U (lazy sums) on every base, count 1 and 3, strided, in place and out of place, the general path
equal to the pseudo-Mersenne path on a base that admits both, and every refusal."""
import ctypes as C

import numpy as np
import pytest

import galois_oracle as go
import keyswitch_sp_oracle as ks
import modswitch_oracle as mo

pytestmark = pytest.mark.gpu

_B = mo.bases(1024)
# name -> (n, primes, switches, pseudo-Mersenne class the kernels must run on: fhe_arith_path & 3)
BASES = {
    "Q4": (1024, _B["Q4"], {}, 1),                                     # the P8192 primes: L = 3, class A
    "Q3": (1024, _B["Q3"], {}, 0),                                     # the P4096 primes: L = 2, general path
    "Q58": (1024, _B["Q58"], {}, 2),                                   # L = 1, class B
    "Q61": (1024, _B["Q61"], {}, 0),                                   # {61-bit, 55-bit}: the special prime is the smaller one
    "Q61R": (1024, _B["Q61R"], {}, 0),                                 # {55-bit, 61-bit}: the larger one
    "S16K": (1024, _B["S16K"], {}, 1),                                 # L = 7
    "Q4-nopm": (1024, _B["Q4"], {"FHE_NTT_NOPM": "1"}, 0),             # the same primes on the general path
    "P8192": (8192, _B["Q4"], {}, 1),                                  # the 13-stage transform
}
OPS = ("relin2", "relin3", "g3", "g2n-1", "gbig")
_cache = {}


def _g_of(op, n):
    return {"g3": 3, "g2n-1": 2 * n - 1, "gbig": pow(3, n // 8, 2 * n)}[op]


def _base(fhe, om, name):
    """(parent ctx, oracle, sk [k][n]) once per base"""
    if name not in _cache:
        n, q, sw, cls = BASES[name]
        ctx = fhe.SEALContext(n, q, go.T_BATCH, switches=sw or None)
        assert (fhe._lib.load().fhe_arith_path(ctx.h) & 3) == cls, name
        rng = np.random.default_rng(17)
        v = rng.integers(0, 3, size=n)
        sk = np.stack([np.where(v == 2, qi - 1, v).astype(np.uint64) for qi in q])
        _cache[name] = (ctx, om.Oracle(n, q, go.T_BATCH), sk)
    return _cache[name]


def _to_lib(fhe, ctx, key_coeff):
    """a coefficient-form key in the library's NTT form"""
    return fhe.Evaluator(ctx).ntt_forward(fhe.to_device(key_coeff, ctx.device))


def _key(fhe, om, name, op):
    """(library key, oracle key) for the operation, a test key under the base's secret"""
    if (name, op) not in _cache:
        ctx, orc, sk = _base(fhe, om, name)
        if op.startswith("relin"):
            target = ks.secret_powers(orc, sk, 2)[int(op[-1]) - 2]
        else:
            target = go.sigma(sk, _g_of(op, ctx.n), ctx.q)
        kc = ks.switch_key(orc, sk, target, seed=len(op) + 3)
        _cache[(name, op)] = (_to_lib(fhe, ctx, kc), ks.key_to_oracle(orc, kc))
    return _cache[(name, op)]


def _p(t):
    return C.c_void_p(t.data_ptr())


def _scratch(fhe, ctx, count):
    import torch
    nbytes = fhe._lib.load().fhe_key_switch_sp_scratch_bytes(ctx.h, count)
    k, L, n = ctx.k, ctx.k - 1, ctx.n
    assert nbytes == count * (L * k + 2 * k + max(L, 2)) * n * 8
    return torch.empty(nbytes // 8, dtype=torch.int64, device=ctx.device), nbytes


def _run(fhe, ctx, op, src, stride, dst, ostride, count, key):
    """one C-ABI call; src / dst flat or shaped device tensors"""
    scr, nbytes = _scratch(fhe, ctx, count)
    if op.startswith("relin"):
        fhe._lib.call("fhe_relinearize_sp_poly", ctx.h, _p(src), stride, int(op[-1]), _p(dst), ostride, count, _p(key), _p(scr), nbytes, None)
    else:
        fhe._lib.call("fhe_apply_galois_sp", ctx.h, _p(src), stride, _p(dst), ostride, count, _g_of(op, ctx.n), _p(key), _p(scr), nbytes, None)


def _want(orc, op, host, korc):
    if op.startswith("relin"):
        return np.stack([ks.relinearize_poly(orc, c, int(op[-1]), korc) for c in host])
    return np.stack([ks.apply_galois(orc, c, _g_of(op, orc.n), korc) for c in host])


def _unreduced(fhe, level, t):
    import torch
    cnt = torch.zeros(1, dtype=torch.int64, device=level.device)
    fhe._lib.call("fhe_count_unreduced", level.h, _p(t), t.numel() // level.n // level.k, _p(cnt), None)
    return int(cnt.cpu()[0])


def _check_all_forms(fhe, ctx, op, host, want, key):
    """out of place (count 3 and 1), in place, strided: all the bytes of `want`; nothing above its modulus; the input untouched"""
    import torch
    count, size = host.shape[:2]
    L, n = ctx.k - 1, ctx.n
    Ln = L * n
    level = ctx.level(L)
    ct = fhe.to_device(host, ctx.device)
    out = torch.full((count, 2, L, n), -1, dtype=torch.int64, device=ctx.device)
    _run(fhe, ctx, op, ct, size * Ln, out, 2 * Ln, count, key)
    got = fhe.to_host(out)
    assert np.array_equal(got, want), (op, np.argwhere(got != want)[:4])
    assert torch.equal(ct, fhe.to_device(host, ctx.device)), "the input was written"
    assert _unreduced(fhe, level, out) == 0
    one = torch.full((1, 2, L, n), -1, dtype=torch.int64, device=ctx.device)
    _run(fhe, ctx, op, ct[count - 1:], size * Ln, one, 2 * Ln, 1, key)
    assert np.array_equal(fhe.to_host(one)[0], want[count - 1]), "count 1 differs"
    buf = ct.clone()                                                    # in place: the same pointer and stride
    _run(fhe, ctx, op, buf, size * Ln, buf, size * Ln, count, key)
    assert np.array_equal(fhe.to_host(buf)[:, :2], want), "in place differs"
    assert torch.equal(buf[:, 2:], ct[:, 2:]), "in place wrote behind the second polynomial"
    si, so = size * Ln + 3 * n, 2 * Ln + 5 * n                          # gaps between the ciphertexts on both sides
    src = torch.full((count, si), -1, dtype=torch.int64, device=ctx.device)
    dst = torch.full((count, so), -1, dtype=torch.int64, device=ctx.device)
    src[:, :size * Ln] = ct.reshape(count, size * Ln)
    _run(fhe, ctx, op, src, si, dst, so, count, key)
    assert np.array_equal(fhe.to_host(dst[:, :2 * Ln].contiguous()).reshape(want.shape), want) and bool((dst[:, 2 * Ln:] == -1).all()), "strided batch differs"


def _operands(ctx, op, seed):
    """[3][size][L][n]: random; family R in the source polynomial (and in c_0 for a rotation); zeros and q_i - 1"""
    q, n, L = ctx.q, ctx.n, ctx.k - 1
    size = int(op[-1]) + 1 if op.startswith("relin") else 2
    rng = np.random.default_rng(seed)
    host = np.stack([np.stack([np.stack([rng.integers(0, qi, size=n, dtype=np.uint64) for qi in q[:L]]) for _ in range(size)]) for _ in range(3)])
    g = None if op.startswith("relin") else _g_of(op, n)
    src = size - 1 if g is None else 1
    host[1, src] = ks.reduction_poly(q, n, g)
    if g is not None:
        host[1, 0] = ks.reduction_poly(q, n, g)
    host[2, src, :, ::2] = 0
    host[2, src, :, 1::4] = np.array(q[:L], dtype=np.uint64)[:, None] - np.uint64(1)
    host[2, 0, :, ::3] = 0
    return host


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name", [b for b in BASES if b != "P8192"])
def test_matches_the_specification(fhe, oracle_mod, name, op):
    ctx, orc, _ = _base(fhe, oracle_mod, name)
    key, korc = _key(fhe, oracle_mod, name, op)
    assert key.numel() == fhe._lib.load().fhe_ksk_sp_words(ctx.h) == (ctx.k - 1) * 2 * ctx.k * ctx.n
    host = _operands(ctx, op, seed=len(name) * 7 + len(op))
    want = _want(orc, op, host, korc)
    _check_all_forms(fhe, ctx, op, host, want, key)
    _cache[("out", name, op)] = want


@pytest.mark.parametrize("op", ["relin2", "g3"])
def test_the_13_stage_transform(fhe, oracle_mod, op):
    """the P8192 preset's own n: the transforms of 8192 points have another barrier structure"""
    ctx, orc, _ = _base(fhe, oracle_mod, "P8192")
    key, korc = _key(fhe, oracle_mod, "P8192", op)
    host = _operands(ctx, op, seed=5)[:2]
    _check_all_forms(fhe, ctx, op, host, _want(orc, op, host, korc), key)


@pytest.mark.parametrize("op", OPS)
def test_general_path_gives_the_pseudo_mersenne_path_s_bytes(fhe, oracle_mod, op):
    """the P8192 primes in a context created with FHE_NTT_NOPM=1 against the default context, the same operands and keys"""
    import torch
    pm, _, _ = _base(fhe, oracle_mod, "Q4")
    gen, _, _ = _base(fhe, oracle_mod, "Q4-nopm")
    key, _ = _key(fhe, oracle_mod, "Q4", op)
    host = _operands(pm, op, seed=99)
    L, n = pm.k - 1, pm.n
    outs = []
    for ctx in (pm, gen):
        ct = fhe.to_device(host, ctx.device)
        out = torch.empty((3, 2, L, n), dtype=torch.int64, device=ctx.device)
        _run(fhe, ctx, op, ct, host.shape[1] * L * n, out, 2 * L * n, 3, key)
        outs.append(out)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("op", ["relin2", "g3", "gbig"])
@pytest.mark.parametrize("name", [b for b in BASES if b != "P8192"])
def test_drop_edges(fhe, oracle_mod, name, op):
    """family D: the source is the constant 1 on residue 0 and 0 elsewhere, key row 0 holds, as data, the transform of
    modswitch_oracle.crafted_tile: the accumulators ARE the tiles, the drop sees every prescribed remainder and final residue, and c_0 / c_1
    hold 0, q_r - 1 and the complements that make the last addmod give exactly 0 and q_r - 1"""
    ctx, orc, _ = _base(fhe, oracle_mod, name)
    q, n, L = ctx.q, ctx.n, ctx.k - 1
    kc = ks.drop_key_rows(orc, ks.drop_tiles(q, n))
    key, korc = _to_lib(fhe, ctx, kc), ks.key_to_oracle(orc, kc)
    unit = ks.unit_source(q, n)
    u = ks.key_switch(orc, unit, korc)
    tiles = ks.drop_tiles(q, n)
    assert np.array_equal(u, np.stack([mo.switch_residues_levels(tiles[pp], q)[L] for pp in range(2)])), "the accumulators are not the tiles"
    add = ks.final_addends(u, q)
    if op.startswith("relin"):
        host = np.stack([add[0], add[1], unit])[None]
    else:
        g = _g_of(op, n)
        host = np.stack([go.sigma(add[0], ks.sigma_inverse(n, g), q[:L]), unit])[None]       # sigma_g(c_0) is the addend; sigma_g(1) = 1
        assert np.array_equal(go.sigma(host[0], g, q[:L]), np.stack([add[0], unit]))
    want = _want(orc, op, host, korc)
    for r in range(L):
        assert set(want[0, 0, r, 2::4]) == {0} and set(want[0, 0, r, 3::4]) == {q[r] - 1}
    host = np.concatenate([host, host, host])
    _check_all_forms(fhe, ctx, op, host, np.concatenate([want, want, want]), key)


@pytest.mark.parametrize("op", ["relin2", "g3"])
@pytest.mark.parametrize("name", ["Q4", "Q58", "S16K", "Q4-nopm"])
def test_lazy_sums(fhe, oracle_mod, name, op):
    """family U: constant source polynomials q_i - 1 and per-slot key residues tau a^-1: each of the L lazy products of every slot of the
    pseudo-Mersenne accumulation is above q_r (tests/test_keyswitch_sp_cpu.py asserts it in the model); Q4-nopm is the control on the
    general path"""
    ctx, orc, _ = _base(fhe, oracle_mod, name)
    q, n, L = ctx.q, ctx.n, ctx.k - 1
    U = ks.Uniform(q, n, pm=BASES[name][3] != 0)
    kc = U.key_coeff(orc)
    key, korc = _to_lib(fhe, ctx, kc), ks.key_to_oracle(orc, kc)
    assert np.array_equal(korc, U.key())
    u = ks.key_switch(orc, U.source(), korc)
    add = ks.final_addends(u, q)
    if op.startswith("relin"):
        host = np.stack([add[0], add[1], U.source()])[None]
    else:
        g = _g_of(op, n)
        host = np.stack([go.sigma(add[0], ks.sigma_inverse(n, g), q[:L]), U.source()])[None]
    host = np.concatenate([host, host, host])
    _check_all_forms(fhe, ctx, op, host, _want(orc, op, host, korc), key)


def test_refusals(fhe, oracle_mod):
    """every FHE_ERR_PARAM condition returns before a launch: the output keeps its sentinel"""
    import torch
    ctx, orc, _ = _base(fhe, oracle_mod, "Q4")
    key, _ = _key(fhe, oracle_mod, "Q4", "relin2")
    gkey, _ = _key(fhe, oracle_mod, "Q4", "g3")
    L, n = ctx.k - 1, ctx.n
    Ln = L * n
    lib = fhe._lib.load()
    ct = ctx.level(L).random_ct(2, size=3)
    out = torch.full((2, 2, L, n), -1, dtype=torch.int64, device=ctx.device)
    scr, nbytes = _scratch(fhe, ctx, 2)
    one = fhe.SEALContext(n, ctx.q[:1], go.T_BATCH)                     # k = 1: no special prime
    p = lambda t: None if t is None else (t if isinstance(t, C.c_void_p) else _p(t))

    def relin(h=ctx.h, src=ct, stride=3 * Ln, sp=2, dst=out, ostride=2 * Ln, count=2, k=key, s=scr, sb=nbytes):
        return lib.fhe_relinearize_sp_poly(h, p(src), stride, sp, p(dst), ostride, count, p(k), p(s), sb, None)

    def gal(h=ctx.h, src=ct, stride=3 * Ln, dst=out, ostride=2 * Ln, count=2, g=3, k=gkey, s=scr, sb=nbytes):
        return lib.fhe_apply_galois_sp(h, p(src), stride, p(dst), ostride, count, g, p(k), p(s), sb, None)

    for call in (relin, gal):
        assert call(h=one.h) == -1 and b"at least 2 primes" in lib.fhe_last_error()
        assert call(h=None) == -1 and call(src=None) == -1 and call(dst=None) == -1 and call(k=None) == -1
        assert call(s=None) == -1 and b"scratch" in lib.fhe_last_error()
        assert call(sb=nbytes - 8) == -1 and b"scratch" in lib.fhe_last_error()
        assert call(ostride=2 * Ln - 1) == -1 and b"stride" in lib.fhe_last_error()
        inside = C.c_void_p(ct.data_ptr() + 8 * Ln)                     # the output inside the input range
        assert call(dst=inside, count=1) == -1 and b"overlaps" in lib.fhe_last_error()
        assert call(dst=ct, ostride=4 * Ln, count=1) == -1              # the same pointer, another stride
        assert call(s=ct) == -1 and b"scratch overlaps" in lib.fhe_last_error()
        assert call(s=out) == -1 and b"scratch overlaps" in lib.fhe_last_error()
        assert call(count=0) == 0 and call(count=0, s=None, sb=0) == 0
    assert relin(sp=1) == -1 and relin(sp=0) == -1 and b"source polynomial" in lib.fhe_last_error()
    assert relin(stride=3 * Ln - 1) == -1 and relin(sp=3) == -1        # a size-3 stride under a source polynomial 3
    assert gal(stride=2 * Ln - 1) == -1
    for g in (4, 1, 0, 2 * n, 2 * n + 1):
        assert gal(g=g) == -1 and b"Galois element" in lib.fhe_last_error()
    assert lib.fhe_ksk_sp_words(one.h) == 0 and lib.fhe_key_switch_sp_scratch_bytes(one.h, 2) == 0
    torch.cuda.synchronize()
    assert bool((out == -1).all()), "a refused call wrote its output"
