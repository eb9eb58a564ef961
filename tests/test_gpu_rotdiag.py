"""GPU: diagonal linear maps on encrypted slots (include/fhe_hip.h fhe_rotate_diag_sum_sp; csrc/rotdiag.hip) against their specification
on the unchanged CPU oracle (tests/rotdiag_oracle.py), bit for bit, through the C ABI: five tap sets and three plaintext families on every
base and path, count 1 and 3, strided, in place and out of place; constant plaintexts equal to fhe_rotate_sum_sp's bytes; the general
path equal to the pseudo-Mersenne path on a base that admits both; the lazy tap sum at 64 taps; the drop's edges; the 13-stage transform;
the FP64 transforms' slot order; every refusal.  Bases, keys and operands are tests/test_gpu_rotsum.py's."""
import ctypes as C

import numpy as np
import pytest

import galois_oracle as go
import keyswitch_sp_oracle as ks
import modswitch_oracle as mo
import rotdiag_oracle as rd
import rotsum_oracle as rs
import test_gpu_rotsum as tg

pytestmark = pytest.mark.gpu

T = tg.T
SMALL = tg.SMALL
_p = tg._p
_fam = {}


def tap_sets(n):
    out = {"id": [1]}
    out.update(tg.tap_sets(n))
    return out


def families(n, G):
    if (n, G) not in _fam:
        _fam[(n, G)] = rd.plain_families(n, T, G, seed=n + G)
    return _fam[(n, G)]


class Plan:
    def __init__(self, fhe, ctx, elts, plains, keys):
        import torch
        self.fhe, self.ctx, self.elts, self.keys = fhe, ctx, list(elts), list(keys)
        e = np.array(elts, dtype=np.uint32)
        self.plains = np.ascontiguousarray(np.stack([np.asarray(p, dtype=np.uint64) for p in plains]))
        assert self.plains.shape == (len(elts), ctx.n)
        kp = (C.c_void_p * len(elts))(*[None if k is None else k.data_ptr() for k in keys])
        self.h = C.c_void_p()
        torch.cuda.synchronize()
        fhe._lib.call("fhe_rotdiag_plan_create", ctx.h, len(elts), e.ctypes.data_as(C.c_void_p), self.plains.ctypes.data_as(C.c_void_p), kp, C.byref(self.h))

    def scratch(self, count):
        import torch
        L, k, n = self.ctx.k - 1, self.ctx.k, self.ctx.n
        nbytes = self.fhe._lib.load().fhe_rotdiag_scratch_bytes(self.h, count)
        assert nbytes == count * (L * k + 3 * k + 2) * n * 8, nbytes
        return torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=self.ctx.device), nbytes

    def sum(self, src, stride, dst, ostride, count):
        scr, nbytes = self.scratch(count)
        self.fhe._lib.call("fhe_rotate_diag_sum_sp", self.h, _p(src), stride, _p(dst), ostride, count, _p(scr), nbytes, None)

    def close(self):
        self.fhe._lib.call("fhe_rotdiag_plan_destroy", self.h)
        self.h = None


def _plan(fhe, om, name, elts, plains):
    ctx, _, _ = tg._base(fhe, om, name)
    pairs = [tg._key(fhe, om, name, g) for g in elts]
    return Plan(fhe, ctx, elts, plains, [p[0] for p in pairs]), [p[1] for p in pairs]


def _out_of_place(fhe, ctx, plan, host):
    import torch
    count, L, n = host.shape[0], ctx.k - 1, ctx.n
    ct = fhe.to_device(host, ctx.device)
    out = torch.full((count, 2, L, n), -1, dtype=torch.int64, device=ctx.device)
    plan.sum(ct, 2 * L * n, out, 2 * L * n, count)
    assert tg._unreduced(fhe, ctx.level(L), out) == 0
    return out


@pytest.mark.parametrize("taps", ["id", "g3", "id+g3", "five", "box3x3"])
@pytest.mark.parametrize("name", SMALL)
def test_matches_the_specification(fhe, oracle_mod, name, taps):
    """random dense plaintexts on three ciphertexts (random; family R in c_1 and c_0; zeros and q_i - 1) in every call shape; (t - 1) X^(n-1)
    and the encoded 0/1 border masks on the first of them, out of place and in place"""
    ctx, orc, _ = tg._base(fhe, oracle_mod, name)
    elts = tap_sets(ctx.n)[taps]
    fam = families(ctx.n, len(elts))
    host = tg._operands(ctx, elts, seed=len(name) * 5 + len(taps))
    for family in ("dense", "top", "mask"):
        plan, korc = _plan(fhe, oracle_mod, name, elts, fam[family])
        if family == "dense":
            want = np.stack([rd.rotate_diag_sum(orc, c, T, elts, fam[family], korc) for c in host])
            tg._check_sum_forms(fhe, ctx, plan, host, want)
        else:
            want = np.stack([rd.rotate_diag_sum(orc, host[0], T, elts, fam[family], korc)])
            got = _out_of_place(fhe, ctx, plan, host[:1])
            assert np.array_equal(fhe.to_host(got), want), (family, np.argwhere(fhe.to_host(got) != want)[:4])
            buf = fhe.to_device(host[:1], ctx.device)
            plan.sum(buf, buf[0].numel(), buf, buf[0].numel(), 1)
            assert np.array_equal(fhe.to_host(buf), want), (family, "in place differs")
        plan.close()


@pytest.mark.parametrize("name", SMALL)
def test_constant_plaintexts_give_rotate_sum_s_bytes(fhe, oracle_mod, name):
    """every p_j a constant polynomial w_j (1, t - 1, (t - 1)/2, (t + 1)/2 among them): the definition is fhe_rotate_sum_sp's"""
    import torch
    ctx, orc, _ = tg._base(fhe, oracle_mod, name)
    n, L = ctx.n, ctx.k - 1
    elts = tap_sets(n)["five"]
    weights = rs.edge_weights(T) + [T - 7]
    plan, korc = _plan(fhe, oracle_mod, name, elts, [rd.constant(n, w) for w in weights])
    ref = tg.Plan(fhe, ctx, elts, weights, plan.keys)
    host = tg._operands(ctx, elts, seed=len(name))
    got = _out_of_place(fhe, ctx, plan, host)
    ct = fhe.to_device(host, ctx.device)
    want = torch.empty_like(got)
    ref.sum(ct, 2 * L * n, want, 2 * L * n, 3)
    assert torch.equal(got, want)
    assert np.array_equal(fhe.to_host(got)[0], rs.rotate_sum(orc, host[0], T, elts, weights, korc))
    plan.close()
    ref.close()


def test_general_path_gives_the_pseudo_mersenne_path_s_bytes(fhe, oracle_mod):
    """the Q4 primes in a context created with FHE_NTT_NOPM=1 against the default context: the same operands, keys, taps and plaintexts"""
    import torch
    pm, _, _ = tg._base(fhe, oracle_mod, "Q4")
    gen, _, _ = tg._base(fhe, oracle_mod, "Q4-nopm")
    elts = tap_sets(pm.n)["box3x3"]
    keys = [tg._key(fhe, oracle_mod, "Q4", g)[0] for g in elts]
    host = tg._operands(pm, elts, seed=98)
    outs = []
    for ctx in (pm, gen):
        for family in ("dense", "mask"):
            plan = Plan(fhe, ctx, elts, families(pm.n, len(elts))[family], keys)
            outs.append(_out_of_place(fhe, ctx, plan, host))
            torch.cuda.synchronize()
            plan.close()
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3])


@pytest.mark.parametrize("name,taps", [("Q58", 64), ("Q4", 64), ("S16K", 8)])
def test_lazy_tap_sums(fhe, oracle_mod, name, taps):
    """rotsum_oracle.TapEdge (every digit product and every weighted tap term of the pseudo-Mersenne accumulation above q_r) with the
    constants +-(t - 1)/2 as plaintexts, 64 taps: fhe_rotate_sum_sp's bytes, and the oracle's"""
    import torch
    ctx, orc, _ = tg._base(fhe, oracle_mod, name)
    q, n, L = ctx.q, ctx.n, ctx.k - 1
    E = rs.TapEdge(q, n, T)
    klib, korc = [], []
    for b in range(2):
        kc = E.key_coeff(orc, b)
        klib.append(tg._to_lib(fhe, ctx, kc))
        korc.append(ks.key_to_oracle(orc, kc))
    elts = rs.many_elements(n, taps)
    weights = [E.weights[j & 1] for j in range(taps)]
    keys = [klib[j & 1] for j in range(taps)]
    plains = [rd.constant(n, w) for w in weights]
    plan = Plan(fhe, ctx, elts, plains, keys)
    rng = np.random.default_rng(taps)
    c0 = np.stack([rng.integers(0, qi, size=n, dtype=np.uint64) for qi in q[:L]])
    host = np.stack([np.stack([c0, E.source()]), np.stack([ks.reduction_poly(q, n, 3), E.source()])])
    want = np.stack([rd.rotate_diag_sum(orc, c, T, elts, plains, [korc[j & 1] for j in range(taps)]) for c in host])
    assert np.array_equal(want[0], rs.rotate_sum(orc, host[0], T, elts, weights, [korc[j & 1] for j in range(taps)]))
    tg._check_sum_forms(fhe, ctx, plan, host, want)
    ref = tg.Plan(fhe, ctx, elts, weights, keys)
    ct = fhe.to_device(host, ctx.device)
    out = torch.empty((2, 2, L, n), dtype=torch.int64, device=ctx.device)
    ref.sum(ct, 2 * L * n, out, 2 * L * n, 2)
    assert np.array_equal(fhe.to_host(out), want)
    plan.close()
    ref.close()


@pytest.mark.parametrize("g", ["g3", "gbig"])
@pytest.mark.parametrize("name", SMALL)
def test_drop_edges(fhe, oracle_mod, name, g):
    """family D of the key switch (tests/test_gpu_rotsum.py test_drop_edges) with the plaintext "1": the accumulators ARE
    modswitch_oracle.crafted_tile, plus p sigma_g(c_0) on the kept residues in the kernels' structure; the drop sees every prescribed
    remainder and final residue, and sigma_g(c_0) holds the addends that make the result exactly 0 and q_r - 1"""
    ctx, orc, _ = tg._base(fhe, oracle_mod, name)
    q, n, L = ctx.q, ctx.n, ctx.k - 1
    g = {"g3": 3, "gbig": pow(3, n // 8, 2 * n)}[g]
    tiles = ks.drop_tiles(q, n)
    kc = ks.drop_key_rows(orc, tiles)
    key, korc = tg._to_lib(fhe, ctx, kc), ks.key_to_oracle(orc, kc)
    unit = ks.unit_source(q, n)
    one = [rd.constant(n, 1)]
    P = rd.transforms(orc, rd.lifts(orc, one, T))
    assert np.array_equal(rd._coeff(orc, rd.accumulators(orc, rs.digits(orc, unit), [g], P, [korc])), tiles), "the accumulators are not the tiles"
    u = np.stack([mo.switch_residues_levels(tiles[pp], q)[L] for pp in range(2)])
    add = ks.final_addends(u, q)
    host = np.stack([go.sigma(add[0], ks.sigma_inverse(n, g), q[:L]), unit])[None]
    want = np.stack([rd.rotate_diag_sum(orc, host[0], T, [g], one, [korc])])
    assert np.array_equal(want[0], rs.rotate_sum(orc, host[0], T, [g], [1], [korc]))
    for r in range(L):
        assert set(want[0, 0, r, 2::4]) == {0} and set(want[0, 0, r, 3::4]) == {q[r] - 1}
    plan = Plan(fhe, ctx, [g], one, [key])
    host = np.concatenate([host, host, host])
    tg._check_sum_forms(fhe, ctx, plan, host, np.concatenate([want, want, want]))
    plan.close()


@pytest.mark.parametrize("name,taps", [("P8192", [1, 3]), ("P4096", [3, 2 * 4096 - 1])])
def test_larger_transforms(fhe, oracle_mod, name, taps):
    """n = 8192 on the Q4 primes (the 13-stage transform) and n = 4096 on the Q3 primes (the FP64 transforms order their slots in their
    own way: P and the permutation tables come from the context's own transform)"""
    ctx, orc, _ = tg._base(fhe, oracle_mod, name)
    rng = np.random.default_rng(ctx.n)
    plains = [rng.integers(0, T, size=ctx.n, dtype=np.uint64) for _ in taps]
    plan, korc = _plan(fhe, oracle_mod, name, taps, plains)
    host = tg._operands(ctx, taps, seed=5, count=1)
    tg._check_sum_forms(fhe, ctx, plan, host, np.stack([rd.rotate_diag_sum(orc, host[0], T, taps, plains, korc)]))
    plan.close()


def test_refusals(fhe, oracle_mod):
    """every FHE_ERR_PARAM condition returns before a launch: the output keeps its sentinel"""
    import torch
    ctx, orc, _ = tg._base(fhe, oracle_mod, "Q4")
    L, n = ctx.k - 1, ctx.n
    Ln = L * n
    lib = fhe._lib.load()
    key3 = tg._key(fhe, oracle_mod, "Q4", 3)[0]
    one = fhe.SEALContext(n, ctx.q[:1], T)                              # k = 1: no special prime
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    ones = lambda G: np.stack([rd.constant(n, j + 1) for j in range(G)])

    def create(h=ctx.h, elts=(1, 3), plains=None, keys=(None, key3), count=None, null_elts=False, null_keys=False, null_plains=False):
        e = np.array(elts, dtype=np.uint32)
        pl = np.ascontiguousarray(ones(max(len(elts), 1)) if plains is None else plains, dtype=np.uint64)
        kp = (C.c_void_p * max(len(elts), 1))(*[None if k is None else k.data_ptr() for k in keys])
        out = C.c_void_p()
        rc = lib.fhe_rotdiag_plan_create(h, len(elts) if count is None else count, None if null_elts else vp(e), None if null_plains else vp(pl),
                                         None if null_keys else kp, C.byref(out))
        if rc == 0:
            lib.fhe_rotdiag_plan_destroy(out)
        return rc

    torch.cuda.synchronize()
    assert create() == 0
    assert create(h=one.h, elts=(3,), keys=(key3,)) == -1 and b"at least 2 primes" in lib.fhe_last_error()
    assert create(count=0) == -1 and b"tap count" in lib.fhe_last_error()
    many = tuple(range(1, 131, 2))
    assert create(elts=many, keys=(key3,) * 65) == -1 and b"tap count" in lib.fhe_last_error()
    for g in (4, 0, 2 * n, 2 * n + 1):
        assert create(elts=(1, g)) == -1 and b"Galois element" in lib.fhe_last_error()
    assert create(elts=(3, 3), keys=(key3, key3)) == -1 and b"repeated" in lib.fhe_last_error()
    bad = ones(2)
    bad[1, n - 1] = T
    assert create(plains=bad) == -1 and b"not below t" in lib.fhe_last_error()
    bad = ones(2)
    bad[0, 0] = 0
    assert create(plains=bad) == -1 and b"zero polynomial" in lib.fhe_last_error()
    assert create(keys=(None, None)) == -1 and b"null key" in lib.fhe_last_error()
    assert create(h=None) == -1 and create(null_elts=True) == -1 and create(null_keys=True) == -1 and create(null_plains=True) == -1
    assert create(keys=(key3, key3)) == 0                               # the key of the tap with g = 1 is ignored

    plan = Plan(fhe, ctx, [1, 3], ones(2), [None, key3])
    ct = ctx.level(L).random_ct(2)
    out = torch.full((2, 2, L, n), -1, dtype=torch.int64, device=ctx.device)
    p = lambda t: None if t is None else (t if isinstance(t, C.c_void_p) else _p(t))
    scr, nbytes = plan.scratch(2)

    def call(h=plan.h, src=ct, stride=2 * Ln, dst=out, ostride=2 * Ln, count=2, s=scr, sb=nbytes):
        return lib.fhe_rotate_diag_sum_sp(h, p(src), stride, p(dst), ostride, count, p(s), sb, None)

    assert call(h=None) == -1 and call(src=None) == -1 and call(dst=None) == -1
    assert call(s=None) == -1 and b"scratch" in lib.fhe_last_error()
    assert call(sb=8) == -1 and b"scratch" in lib.fhe_last_error()
    assert call(sb=nbytes - 8) == -1 and b"scratch" in lib.fhe_last_error()
    assert call(stride=2 * Ln - 1) == -1 and b"stride" in lib.fhe_last_error()
    assert call(ostride=2 * Ln - 1) == -1 and b"stride" in lib.fhe_last_error()
    inside = C.c_void_p(ct.data_ptr() + 8 * Ln)                         # the output inside the input range
    assert call(dst=inside, count=1) == -1 and b"overlaps" in lib.fhe_last_error()
    big = torch.empty((2, 3 * Ln), dtype=torch.int64, device=ctx.device)
    assert call(src=big, stride=3 * Ln, dst=big, ostride=2 * Ln) == -1 and b"overlaps" in lib.fhe_last_error()      # the same pointer, another stride
    assert call(s=ct) == -1 and b"scratch overlaps" in lib.fhe_last_error()
    assert call(s=out) == -1 and b"scratch overlaps" in lib.fhe_last_error()
    assert call(count=0) == 0 and call(count=0, s=None, sb=0) == 0
    assert lib.fhe_rotdiag_scratch_bytes(None, 2) == 0
    torch.cuda.synchronize()
    assert bool((out == -1).all()), "a refused call wrote its output"
    buf = ct.clone()
    assert call(src=buf, dst=buf) == 0                                  # in place is allowed
    torch.cuda.synchronize()
    plan.close()
