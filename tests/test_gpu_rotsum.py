"""GPU: the hoisted special-prime rotations (include/fhe_hip.h fhe_rotate_sum_sp / fhe_rotate_each_sp; csrc/rotsum.hip) against their
specification on the unchanged CPU oracle (tests/rotsum_oracle.py), bit for bit, through the C ABI: four tap sets with the edge weights on
every base and path, count 1 and 3, strided, in place and out of place, the separate outputs, the general path equal to the
pseudo-Mersenne path on a base that admits both, the lazy tap sum at 64 taps, the drop's edges, the 13-stage transform, the FP64
transforms' slot order, and every refusal."""
import ctypes as C

import numpy as np
import pytest

import galois_oracle as go
import keyswitch_sp_oracle as ks
import modswitch_oracle as mo
import rotsum_oracle as rs

pytestmark = pytest.mark.gpu

T = go.T_BATCH
_B = mo.bases(1024)
# name -> (n, primes, switches, pseudo-Mersenne class the kernels must run on: fhe_arith_path & 3): tests/test_gpu_keyswitch_sp.py's
BASES = {
    "Q4": (1024, _B["Q4"], {}, 1),
    "Q3": (1024, _B["Q3"], {}, 0),
    "Q58": (1024, _B["Q58"], {}, 2),
    "Q61": (1024, _B["Q61"], {}, 0),
    "Q61R": (1024, _B["Q61R"], {}, 0),
    "S16K": (1024, _B["S16K"], {}, 1),
    "Q4-nopm": (1024, _B["Q4"], {"FHE_NTT_NOPM": "1"}, 0),
    "P8192": (8192, _B["Q4"], {}, 1),                                  # the 13-stage transform
    "P4096": (4096, _B["Q3"], {}, 0),                                  # the P4096 preset: the FP64 transforms' slot order
}
SMALL = [b for b in BASES if BASES[b][0] == 1024]
_cache = {}


def tap_sets(n):
    return {"g3": [3], "id+g3": [1, 3], "five": [1, 3, 2 * n - 1, pow(3, n // 8, 2 * n), pow(3, -1, 2 * n)], "box3x3": rs.filter_elements(n, 32, 3, 3)}


def weights_for(elts):
    """the edge weights 1, t - 1, (t - 1)/2, (t + 1)/2 first, then others on both sides of t/2"""
    pool = rs.edge_weights(T) + [2, T - 7, 255, T - 256, 40000]
    return [pool[j % len(pool)] for j in range(len(elts))]


def _base(fhe, om, name):
    if name not in _cache:
        n, q, sw, cls = BASES[name]
        ctx = fhe.SEALContext(n, q, T, switches=sw or None)
        assert (fhe._lib.load().fhe_arith_path(ctx.h) & 3) == cls, name
        rng = np.random.default_rng(17)
        v = rng.integers(0, 3, size=n)
        sk = np.stack([np.where(v == 2, qi - 1, v).astype(np.uint64) for qi in q])
        _cache[name] = (ctx, om.Oracle(n, q, T), sk)
    return _cache[name]


def _to_lib(fhe, ctx, key_coeff):
    return fhe.Evaluator(ctx).ntt_forward(fhe.to_device(key_coeff, ctx.device))


def _key(fhe, om, name, g):
    """(library key, oracle key) for sigma_g(s), a test key under the base's secret; (None, None) for g = 1"""
    if g == 1:
        return None, None
    if (name, g) not in _cache:
        ctx, orc, sk = _base(fhe, om, name)
        kc = ks.switch_key(orc, sk, go.sigma(sk, g, ctx.q), seed=g % 1000 + 3)
        _cache[(name, g)] = (_to_lib(fhe, ctx, kc), ks.key_to_oracle(orc, kc))
    return _cache[(name, g)]


def _p(t):
    return C.c_void_p(t.data_ptr())


class Plan:
    def __init__(self, fhe, ctx, elts, weights, keys):
        import torch
        self.fhe, self.ctx, self.elts, self.keys = fhe, ctx, list(elts), list(keys)
        e = np.array(elts, dtype=np.uint32)
        w = None if weights is None else np.array([int(x) for x in weights], dtype=np.uint64)
        kp = (C.c_void_p * len(elts))(*[None if k is None else k.data_ptr() for k in keys])
        self.h = C.c_void_p()
        torch.cuda.synchronize()
        fhe._lib.call("fhe_rotsum_plan_create", ctx.h, len(elts), e.ctypes.data_as(C.c_void_p), None if w is None else w.ctypes.data_as(C.c_void_p), kp, C.byref(self.h))

    def scratch(self, count, each=False):
        import torch
        L, k, n, G = self.ctx.k - 1, self.ctx.k, self.ctx.n, len(self.elts)
        R = max(1, sum(g != 1 for g in self.elts))
        nbytes = self.fhe._lib.load().fhe_rotsum_scratch_bytes(self.h, count, int(each))
        assert nbytes == (count * (L * k + R * 2 * k + max(2 * R, L)) * n * 8 if each else count * (L * k + 2 * k + 2 * L) * n * 8), (nbytes, G)
        return torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=self.ctx.device), nbytes

    def sum(self, src, stride, dst, ostride, count):
        scr, nbytes = self.scratch(count)
        self.fhe._lib.call("fhe_rotate_sum_sp", self.h, _p(src), stride, _p(dst), ostride, count, _p(scr), nbytes, None)

    def each(self, src, stride, dst, ostride, tstride, count):
        scr, nbytes = self.scratch(count, each=True)
        self.fhe._lib.call("fhe_rotate_each_sp", self.h, _p(src), stride, _p(dst), ostride, tstride, count, _p(scr), nbytes, None)

    def close(self):
        self.fhe._lib.call("fhe_rotsum_plan_destroy", self.h)
        self.h = None


def _plan(fhe, om, name, elts, weights):
    ctx, _, _ = _base(fhe, om, name)
    pairs = [_key(fhe, om, name, g) for g in elts]
    return Plan(fhe, ctx, elts, weights, [p[0] for p in pairs]), [p[1] for p in pairs]


def _unreduced(fhe, level, t):
    import torch
    cnt = torch.zeros(1, dtype=torch.int64, device=level.device)
    fhe._lib.call("fhe_count_unreduced", level.h, _p(t), t.numel() // level.n // level.k, _p(cnt), None)
    return int(cnt.cpu()[0])


def _check_sum_forms(fhe, ctx, plan, host, want):
    """out of place (the whole batch and its last ciphertext alone), in place, strided: all the bytes of `want`; nothing above its modulus;
    the input untouched"""
    import torch
    count = host.shape[0]
    L, n = ctx.k - 1, ctx.n
    Ln = L * n
    level = ctx.level(L)
    ct = fhe.to_device(host, ctx.device)
    out = torch.full((count, 2, L, n), -1, dtype=torch.int64, device=ctx.device)
    plan.sum(ct, 2 * Ln, out, 2 * Ln, count)
    got = fhe.to_host(out)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert torch.equal(ct, fhe.to_device(host, ctx.device)), "the input was written"
    assert _unreduced(fhe, level, out) == 0
    if count > 1:
        one = torch.full((1, 2, L, n), -1, dtype=torch.int64, device=ctx.device)
        plan.sum(ct[count - 1:], 2 * Ln, one, 2 * Ln, 1)
        assert np.array_equal(fhe.to_host(one)[0], want[count - 1]), "count 1 differs"
    buf = ct.clone()                                                    # in place: the same pointer and stride
    plan.sum(buf, 2 * Ln, buf, 2 * Ln, count)
    assert np.array_equal(fhe.to_host(buf), want), "in place differs"
    si, so = 2 * Ln + 3 * n, 2 * Ln + 5 * n                             # gaps between the ciphertexts on both sides
    src = torch.full((count, si), -1, dtype=torch.int64, device=ctx.device)
    dst = torch.full((count, so), -1, dtype=torch.int64, device=ctx.device)
    src[:, :2 * Ln] = ct.reshape(count, 2 * Ln)
    plan.sum(src, si, dst, so, count)
    assert np.array_equal(fhe.to_host(dst[:, :2 * Ln].contiguous()).reshape(want.shape), want) and bool((dst[:, 2 * Ln:] == -1).all()), "strided batch differs"
    buf = src.clone()                                                   # in place and strided
    plan.sum(buf, si, buf, si, count)
    assert np.array_equal(fhe.to_host(buf[:, :2 * Ln].contiguous()).reshape(want.shape), want) and bool((buf[:, 2 * Ln:] == -1).all()), "strided in place differs"


def _check_each(fhe, ctx, plan, host, want):
    """want [G][count][2][L][n]: contiguous and strided (gaps between the ciphertexts and between the taps)"""
    import torch
    count, G = host.shape[0], len(plan.elts)
    L, n = ctx.k - 1, ctx.n
    Ln = L * n
    level = ctx.level(L)
    ct = fhe.to_device(host, ctx.device)
    out = torch.full((G, count, 2, L, n), -1, dtype=torch.int64, device=ctx.device)
    plan.each(ct, 2 * Ln, out, 2 * Ln, count * 2 * Ln, count)
    got = fhe.to_host(out)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert torch.equal(ct, fhe.to_device(host, ctx.device)), "the input was written"
    assert _unreduced(fhe, level, out) == 0
    so = 2 * Ln + 3 * n
    ts = count * so + 7 * n
    dst = torch.full((G, ts), -1, dtype=torch.int64, device=ctx.device)
    plan.each(ct, 2 * Ln, dst, so, ts, count)
    body = dst[:, :count * so].reshape(G, count, so)
    assert np.array_equal(fhe.to_host(body[:, :, :2 * Ln].contiguous()).reshape(want.shape), want), "strided outputs differ"
    assert bool((body[:, :, 2 * Ln:] == -1).all()) and bool((dst[:, count * so:] == -1).all()), "a gap was written"


def _operands(ctx, elts, seed, count=3):
    """[count][2][L][n]: random; family R (keyswitch_sp_oracle.reduction_poly) in c_1 and c_0; zeros and q_i - 1"""
    q, n, L = ctx.q, ctx.n, ctx.k - 1
    rng = np.random.default_rng(seed)
    host = np.stack([np.stack([np.stack([rng.integers(0, qi, size=n, dtype=np.uint64) for qi in q[:L]]) for _ in range(2)]) for _ in range(count)])
    g = next((e for e in elts if e != 1), 3)
    if count > 1:
        host[1, 1] = ks.reduction_poly(q, n, g)
        host[1, 0] = ks.reduction_poly(q, n, g)
    if count > 2:
        host[2, 1, :, ::2] = 0
        host[2, 1, :, 1::4] = np.array(q[:L], dtype=np.uint64)[:, None] - np.uint64(1)
        host[2, 0, :, ::3] = 0
    return host


@pytest.mark.parametrize("taps", ["g3", "id+g3", "five", "box3x3"])
@pytest.mark.parametrize("name", SMALL)
def test_matches_the_specification(fhe, oracle_mod, name, taps):
    ctx, orc, _ = _base(fhe, oracle_mod, name)
    elts = tap_sets(ctx.n)[taps]
    weights = weights_for(elts)
    plan, korc = _plan(fhe, oracle_mod, name, elts, weights)
    host = _operands(ctx, elts, seed=len(name) * 7 + len(taps))
    want = np.stack([rs.rotate_sum(orc, c, T, elts, weights, korc) for c in host])
    _check_sum_forms(fhe, ctx, plan, host, want)
    if taps in ("id+g3", "five"):
        each = np.stack([rs.rotate_each(orc, c, T, elts, korc) for c in host], axis=1)
        _check_each(fhe, ctx, plan, host, each)
        if taps == "id+g3":                                             # NOT the op-by-op rotation's bits (include/fhe_hip.h)
            assert not np.array_equal(each[1, 0], ks.apply_galois(orc, host[0], 3, korc[1]))
    plan.close()


def test_null_weights_are_ones(fhe, oracle_mod):
    ctx, orc, _ = _base(fhe, oracle_mod, "Q4")
    elts = tap_sets(ctx.n)["id+g3"]
    pairs = [_key(fhe, oracle_mod, "Q4", g) for g in elts]
    plan = Plan(fhe, ctx, elts, None, [p[0] for p in pairs])
    host = _operands(ctx, elts, seed=4, count=1)
    _check_sum_forms(fhe, ctx, plan, host, np.stack([rs.rotate_sum(orc, host[0], T, elts, [1, 1], [p[1] for p in pairs])]))
    plan.close()


@pytest.mark.parametrize("name,taps", [("P8192", [1, 3]), ("P4096", [3, 2 * 4096 - 1])])
def test_larger_transforms(fhe, oracle_mod, name, taps):
    """n = 8192 on the P8192 primes (the 13-stage transform) and n = 4096 on the P4096 primes (the FP64 transforms order their slots in
    their own way: the permutation tables come from the context's own transform of X)"""
    ctx, orc, _ = _base(fhe, oracle_mod, name)
    weights = [T - 1, (T + 1) // 2]
    plan, korc = _plan(fhe, oracle_mod, name, taps, weights)
    host = _operands(ctx, taps, seed=5, count=1)
    _check_sum_forms(fhe, ctx, plan, host, np.stack([rs.rotate_sum(orc, host[0], T, taps, weights, korc)]))
    _check_each(fhe, ctx, plan, host, np.stack([rs.rotate_each(orc, host[0], T, taps, korc)], axis=1))
    plan.close()


def test_general_path_gives_the_pseudo_mersenne_path_s_bytes(fhe, oracle_mod):
    """the P8192 primes in a context created with FHE_NTT_NOPM=1 against the default context: the same operands, keys and taps"""
    import torch
    pm, _, _ = _base(fhe, oracle_mod, "Q4")
    gen, _, _ = _base(fhe, oracle_mod, "Q4-nopm")
    elts = tap_sets(pm.n)["five"]
    weights = weights_for(elts)
    keys = [_key(fhe, oracle_mod, "Q4", g)[0] for g in elts]
    host = _operands(pm, elts, seed=99)
    L, n = pm.k - 1, pm.n
    sums, eachs = [], []
    for ctx in (pm, gen):
        plan = Plan(fhe, ctx, elts, weights, keys)
        ct = fhe.to_device(host, ctx.device)
        out = torch.empty((3, 2, L, n), dtype=torch.int64, device=ctx.device)
        plan.sum(ct, 2 * L * n, out, 2 * L * n, 3)
        each = torch.empty((len(elts), 3, 2, L, n), dtype=torch.int64, device=ctx.device)
        plan.each(ct, 2 * L * n, each, 2 * L * n, 3 * 2 * L * n, 3)
        sums.append(out)
        eachs.append(each)
        torch.cuda.synchronize()
        plan.close()
    assert torch.equal(sums[0], sums[1]) and torch.equal(eachs[0], eachs[1])


@pytest.mark.parametrize("name,taps", [("Q58", 64), ("Q4", 64), ("S16K", 8)])
def test_lazy_tap_sums(fhe, oracle_mod, name, taps):
    """family U extended over taps (rotsum_oracle.TapEdge): constant sources q_i - 1 and per-slot key residues for which every digit product
    AND every weighted tap term of the pseudo-Mersenne accumulation is above q_r, 64 taps of weight +-(t - 1)/2 (S16K: 8 taps, its oracle
    side is Python over 8 primes); tests/test_rotsum_cpu.py shows in the model that the 64-tap sum on the 58-bit base wraps without its fold"""
    ctx, orc, _ = _base(fhe, oracle_mod, name)
    q, n, L = ctx.q, ctx.n, ctx.k - 1
    E = rs.TapEdge(q, n, T)
    klib, korc = [], []
    for b in range(2):
        kc = E.key_coeff(orc, b)
        klib.append(_to_lib(fhe, ctx, kc))
        korc.append(ks.key_to_oracle(orc, kc))
        assert np.array_equal(korc[b], E.key(b))
    elts = rs.many_elements(n, taps)
    weights = [E.weights[j & 1] for j in range(taps)]
    plan = Plan(fhe, ctx, elts, weights, [klib[j & 1] for j in range(taps)])
    rng = np.random.default_rng(taps)
    c0 = np.stack([rng.integers(0, qi, size=n, dtype=np.uint64) for qi in q[:L]])
    host = np.stack([np.stack([c0, E.source()]), np.stack([ks.reduction_poly(q, n, 3), E.source()])])
    want = np.stack([rs.rotate_sum(orc, c, T, elts, weights, [korc[j & 1] for j in range(taps)]) for c in host])
    _check_sum_forms(fhe, ctx, plan, host, want)
    plan.close()


@pytest.mark.parametrize("g", ["g3", "gbig"])
@pytest.mark.parametrize("name", SMALL)
def test_drop_edges(fhe, oracle_mod, name, g):
    """family D of the key switch: c_1 is the constant 1 on residue 0, key row 0 holds, as data, modswitch_oracle.crafted_tile: with one tap
    of weight 1 the accumulators ARE the tiles (a slot permutation leaves the transform of a constant alone), the drop sees every
    prescribed remainder and final residue, and sigma_g(c_0) holds the addends that make the last addmod give exactly 0 and q_r - 1"""
    ctx, orc, _ = _base(fhe, oracle_mod, name)
    q, n, L = ctx.q, ctx.n, ctx.k - 1
    g = {"g3": 3, "gbig": pow(3, n // 8, 2 * n)}[g]
    tiles = ks.drop_tiles(q, n)
    kc = ks.drop_key_rows(orc, tiles)
    key, korc = _to_lib(fhe, ctx, kc), ks.key_to_oracle(orc, kc)
    unit = ks.unit_source(q, n)
    acc = rs.accumulators(orc, rs.digits(orc, unit), [g], [1], [korc])
    assert np.array_equal(acc, tiles), "the accumulators are not the tiles"
    u = np.stack([mo.switch_residues_levels(tiles[pp], q)[L] for pp in range(2)])
    add = ks.final_addends(u, q)
    host = np.stack([go.sigma(add[0], ks.sigma_inverse(n, g), q[:L]), unit])[None]
    want = np.stack([rs.rotate_sum(orc, host[0], T, [g], [1], [korc])])
    for r in range(L):
        assert set(want[0, 0, r, 2::4]) == {0} and set(want[0, 0, r, 3::4]) == {q[r] - 1}
    plan = Plan(fhe, ctx, [g], [1], [key])
    host = np.concatenate([host, host, host])
    _check_sum_forms(fhe, ctx, plan, host, np.concatenate([want, want, want]))
    _check_each(fhe, ctx, plan, host, np.concatenate([want, want, want])[None])
    plan.close()


def test_refusals(fhe, oracle_mod):
    """every FHE_ERR_PARAM condition returns before a launch: the output keeps its sentinel"""
    import torch
    ctx, orc, _ = _base(fhe, oracle_mod, "Q4")
    L, n = ctx.k - 1, ctx.n
    Ln = L * n
    lib = fhe._lib.load()
    key3 = _key(fhe, oracle_mod, "Q4", 3)[0]
    one = fhe.SEALContext(n, ctx.q[:1], T)                              # k = 1: no special prime
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def create(h=ctx.h, elts=(1, 3), weights=(1, 2), keys=(None, key3), count=None, null_elts=False, null_keys=False):
        e, w = np.array(elts, dtype=np.uint32), np.array(weights, dtype=np.uint64)
        kp = (C.c_void_p * max(len(elts), 1))(*[None if k is None else k.data_ptr() for k in keys])
        out = C.c_void_p()
        rc = lib.fhe_rotsum_plan_create(h, len(elts) if count is None else count, None if null_elts else vp(e), vp(w), None if null_keys else kp, C.byref(out))
        if rc == 0:
            lib.fhe_rotsum_plan_destroy(out)
        return rc

    torch.cuda.synchronize()
    assert create() == 0
    assert create(h=one.h, elts=(3,), weights=(1,), keys=(key3,)) == -1 and b"at least 2 primes" in lib.fhe_last_error()
    assert create(count=0) == -1 and b"tap count" in lib.fhe_last_error()
    many = tuple(range(1, 131, 2))
    assert create(elts=many, weights=(1,) * 65, keys=(key3,) * 65) == -1 and b"tap count" in lib.fhe_last_error()
    for g in (4, 0, 2 * n, 2 * n + 1):
        assert create(elts=(1, g)) == -1 and b"Galois element" in lib.fhe_last_error()
    assert create(elts=(3, 3), keys=(key3, key3)) == -1 and b"repeated" in lib.fhe_last_error()
    assert create(weights=(1, T)) == -1 and create(weights=(0, 1)) == -1 and b"0 modulo t" in lib.fhe_last_error()
    assert create(keys=(None, None)) == -1 and b"null key" in lib.fhe_last_error()
    assert create(h=None) == -1 and create(null_elts=True) == -1 and create(null_keys=True) == -1
    assert create(keys=(key3, key3)) == 0                               # the key of the tap with g = 1 is ignored

    plan = Plan(fhe, ctx, [1, 3], [1, 2], [None, key3])
    ct = ctx.level(L).random_ct(2)
    out = torch.full((2, 2, 2, L, n), -1, dtype=torch.int64, device=ctx.device)
    p = lambda t: None if t is None else (t if isinstance(t, C.c_void_p) else _p(t))
    scr, nbytes = plan.scratch(2)
    scre, nbe = plan.scratch(2, each=True)

    def rsum(h=plan.h, src=ct, stride=2 * Ln, dst=out, ostride=2 * Ln, count=2, s=scr, sb=nbytes):
        return lib.fhe_rotate_sum_sp(h, p(src), stride, p(dst), ostride, count, p(s), sb, None)

    def each(h=plan.h, src=ct, stride=2 * Ln, dst=out, ostride=2 * Ln, tstride=2 * 2 * Ln, count=2, s=scre, sb=nbe):
        return lib.fhe_rotate_each_sp(h, p(src), stride, p(dst), ostride, tstride, count, p(s), sb, None)

    for call in (rsum, each):
        assert call(h=None) == -1 and call(src=None) == -1 and call(dst=None) == -1
        assert call(s=None) == -1 and b"scratch" in lib.fhe_last_error()
        assert call(sb=8) == -1 and b"scratch" in lib.fhe_last_error()
        assert call(stride=2 * Ln - 1) == -1 and b"stride" in lib.fhe_last_error()
        assert call(ostride=2 * Ln - 1) == -1 and b"stride" in lib.fhe_last_error()
        inside = C.c_void_p(ct.data_ptr() + 8 * Ln)                     # the output inside the input range
        assert call(dst=inside, count=1) == -1 and b"overlaps" in lib.fhe_last_error()
        assert call(dst=ct, ostride=3 * Ln, count=1) == -1              # the same pointer, another stride
        assert call(s=ct) == -1 and b"scratch overlaps" in lib.fhe_last_error()
        assert call(s=out) == -1 and b"scratch overlaps" in lib.fhe_last_error()
        assert call(count=0) == 0 and call(count=0, s=None, sb=0) == 0
    assert rsum(sb=nbytes - 8) == -1 and each(sb=nbe - 8) == -1
    assert each(dst=ct) == -1 and b"no in-place form" in lib.fhe_last_error()
    assert each(tstride=2 * 2 * Ln - 1) == -1 and b"tap stride" in lib.fhe_last_error()
    assert lib.fhe_rotsum_scratch_bytes(None, 2, 0) == 0
    torch.cuda.synchronize()
    assert bool((out == -1).all()), "a refused call wrote its output"
    buf = ct.clone()
    assert rsum(src=buf, dst=buf) == 0                                  # in place is allowed for the sum
    plan.close()
