"""GPU: baby-step / giant-step linear maps on encrypted slots (include/fhe_hip.h fhe_rotate_bsgs_sp; csrc/rotbsgs.hip) against their
specification on the unchanged CPU oracle (tests/rotbsgs_oracle.py), bit for bit, through the C ABI: six shapes (G1, G2) and three
plaintext families on every base and path, count 1 and 3, strided, in place and out of place; the two byte identities against
fhe_rotate_diag_sum_sp and fhe_rotate_sum_sp on the device; the general path equal to the pseudo-Mersenne path on a base that admits
both; the lazy sums' fold points at (64, 64); the drop's edges at both drops; the scratch formula; every refusal; the larger transforms.
Bases, keys and operands are tests/test_gpu_rotsum.py's."""
import ctypes as C

import numpy as np
import pytest

import galois_oracle as go
import keyswitch_sp_oracle as ks
import modswitch_oracle as mo
import rotbsgs_oracle as ro
import rotdiag_oracle as rd
import rotsum_oracle as rs
import test_gpu_rotdiag as tdg
import test_gpu_rotsum as tg

pytestmark = pytest.mark.gpu

T = tg.T
SMALL = tg.SMALL
_p = tg._p
_fam = {}


def shapes(n):
    """name -> (baby, giant, absent pairs)"""
    e = lambda s: pow(3, s % (n // 2), 2 * n)
    return {
        "1x1": ([3], [2 * n - 1], ()),
        "3x1-id": ([1, 3, 2 * n - 1], [1], ()),
        "1x2": ([1], [3, e(-1)], ()),
        "4x3": ([1, 3, e(2), e(3)], [e(4), 1, e(-4)], ()),
        "4x3-absent": ([1, 3, e(2), e(3)], [e(4), 1, e(-4)], ((0, 0), (1, 2), (1, 3), (2, 1))),
        "16x8": ([e(j) for j in range(16)], [e(16 * a) for a in range(-4, 4)], ()),
    }


def families(n, G1, G2, absent=()):
    key = (n, G1, G2, tuple(absent))
    if key not in _fam:
        _fam[key] = ro.plain_families(n, T, G1, G2, seed=n + G1 + 64 * G2, absent=absent)
    return _fam[key]


class Plan:
    def __init__(self, fhe, ctx, baby, giant, plains, kb, kg):
        import torch
        self.fhe, self.ctx, self.baby, self.giant, self.keys = fhe, ctx, list(baby), list(giant), (list(kb), list(kg))
        eb, eg = np.array(baby, dtype=np.uint32), np.array(giant, dtype=np.uint32)
        self.plains = np.ascontiguousarray(np.asarray(plains, dtype=np.uint64))
        assert self.plains.shape == (len(giant), len(baby), ctx.n)
        pb = (C.c_void_p * len(baby))(*[None if k is None else k.data_ptr() for k in kb])
        pg = (C.c_void_p * len(giant))(*[None if k is None else k.data_ptr() for k in kg])
        self.h = C.c_void_p()
        torch.cuda.synchronize()
        fhe._lib.call("fhe_rotbsgs_plan_create", ctx.h, len(baby), eb.ctypes.data_as(C.c_void_p), len(giant), eg.ctypes.data_as(C.c_void_p),
                      self.plains.ctypes.data_as(C.c_void_p), pb, pg, C.byref(self.h))

    def scratch(self, count):
        """the formula include/fhe_hip.h documents"""
        import torch
        L, k, n, G2 = self.ctx.k - 1, self.ctx.k, self.ctx.n, len(self.giant)
        nbytes = self.fhe._lib.load().fhe_rotbsgs_scratch_bytes(self.h, count)
        assert nbytes == 8 * count * n * ((L * k + 3 * k + 2) + G2 * (2 * k + 1 + L + L * k)), nbytes
        return torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=self.ctx.device), nbytes

    def sum(self, src, stride, dst, ostride, count):
        scr, nbytes = self.scratch(count)
        self.fhe._lib.call("fhe_rotate_bsgs_sp", self.h, _p(src), stride, _p(dst), ostride, count, _p(scr), nbytes, None)

    def close(self):
        self.fhe._lib.call("fhe_rotbsgs_plan_destroy", self.h)
        self.h = None


def _plan(fhe, om, name, baby, giant, plains):
    """(plan, oracle keys of the baby list, of the giant list)"""
    ctx, _, _ = tg._base(fhe, om, name)
    pb = [tg._key(fhe, om, name, g) for g in baby]
    pg = [tg._key(fhe, om, name, g) for g in giant]
    return Plan(fhe, ctx, baby, giant, plains, [p[0] for p in pb], [p[0] for p in pg]), [p[1] for p in pb], [p[1] for p in pg]


def _check_one(fhe, ctx, plan, host, want, what):
    """one ciphertext out of place and in place"""
    got = tdg._out_of_place(fhe, ctx, plan, host)
    assert np.array_equal(fhe.to_host(got), want), (what, np.argwhere(fhe.to_host(got) != want)[:4])
    buf = fhe.to_device(host, ctx.device)
    plan.sum(buf, buf[0].numel(), buf, buf[0].numel(), host.shape[0])
    assert np.array_equal(fhe.to_host(buf), want), (what, "in place differs")


@pytest.mark.parametrize("shape", ["1x1", "3x1-id", "1x2", "4x3", "4x3-absent", "16x8"])
@pytest.mark.parametrize("name", SMALL)
def test_matches_the_specification(fhe, oracle_mod, name, shape):
    """random dense plaintexts on three ciphertexts (random; family R in c_1 and c_0; zeros and q_i - 1) in every call shape; (t - 1) X^(n-1)
    and the encoded 0/1 border masks on the first of them, out of place and in place"""
    ctx, orc, _ = tg._base(fhe, oracle_mod, name)
    baby, giant, absent = shapes(ctx.n)[shape]
    fam = families(ctx.n, len(baby), len(giant), absent)
    host = tg._operands(ctx, [g for g in baby + giant if g != 1], seed=len(name) * 5 + len(shape))
    for family in ("dense", "top", "mask"):
        plan, kb, kg = _plan(fhe, oracle_mod, name, baby, giant, fam[family])
        if family == "dense":
            want = np.stack([ro.rotate_bsgs(orc, c, T, baby, giant, fam[family], kb, kg) for c in host])
            tg._check_sum_forms(fhe, ctx, plan, host, want)
        else:
            want = np.stack([ro.rotate_bsgs(orc, host[0], T, baby, giant, fam[family], kb, kg)])
            _check_one(fhe, ctx, plan, host[:1], want, family)
        plan.close()


@pytest.mark.parametrize("name", SMALL)
def test_byte_identities_on_the_device(fhe, oracle_mod, name):
    """G2 = 1, h = {1}: fhe_rotate_diag_sum_sp's bytes on the taps (g_j, p_(0,j)); G1 = 1, g = {1}, p = 1 and one giant h != 1:
    fhe_rotate_sum_sp's bytes for the tap set {h} with weight 1"""
    import torch
    ctx, orc, _ = tg._base(fhe, oracle_mod, name)
    n, L = ctx.n, ctx.k - 1
    elts = tg.tap_sets(n)["five"]
    host = tg._operands(ctx, elts, seed=len(name) + 1)
    ct = fhe.to_device(host, ctx.device)
    for family in ("dense", "mask"):
        plains = tdg.families(n, len(elts))[family]
        plan, kb, _ = _plan(fhe, oracle_mod, name, elts, [1], np.stack(plains)[None])
        ref = tdg.Plan(fhe, ctx, elts, plains, plan.keys[0])
        got = tdg._out_of_place(fhe, ctx, plan, host)
        want = torch.empty_like(got)
        ref.sum(ct, 2 * L * n, want, 2 * L * n, 3)
        assert torch.equal(got, want), family
        plan.close()
        ref.close()
    assert np.array_equal(fhe.to_host(got)[0], rd.rotate_diag_sum(orc, host[0], T, elts, plains, kb))
    for h in elts[1:3]:
        plan, _, kg = _plan(fhe, oracle_mod, name, [1], [h], rd.constant(n, 1)[None, None])
        ref = tg.Plan(fhe, ctx, [h], [1], plan.keys[1])
        got = tdg._out_of_place(fhe, ctx, plan, host)
        want = torch.empty_like(got)
        ref.sum(ct, 2 * L * n, want, 2 * L * n, 3)
        assert torch.equal(got, want), h
        plan.close()
        ref.close()


def test_general_path_gives_the_pseudo_mersenne_path_s_bytes(fhe, oracle_mod):
    """the Q4 primes in a context created with FHE_NTT_NOPM=1 against the default context: the same operands, keys, lists and plaintexts"""
    import torch
    pm, _, _ = tg._base(fhe, oracle_mod, "Q4")
    gen, _, _ = tg._base(fhe, oracle_mod, "Q4-nopm")
    outs = []
    for shape in ("4x3-absent", "16x8"):
        baby, giant, absent = shapes(pm.n)[shape]
        kb = [tg._key(fhe, oracle_mod, "Q4", g)[0] for g in baby]
        kg = [tg._key(fhe, oracle_mod, "Q4", g)[0] for g in giant]
        host = tg._operands(pm, [3], seed=97)
        for ctx in (pm, gen):
            for family in ("dense", "mask"):
                plan = Plan(fhe, ctx, baby, giant, families(pm.n, len(baby), len(giant), absent)[family], kb, kg)
                outs.append(tdg._out_of_place(fhe, ctx, plan, host))
                torch.cuda.synchronize()
                plan.close()
    for b in (0, 4):
        assert torch.equal(outs[b], outs[b + 2]) and torch.equal(outs[b + 1], outs[b + 3])


@pytest.mark.parametrize("name", ["Q58", "Q4"])
def test_lazy_sums_at_64_by_64(fhe, oracle_mod, name):
    """rotsum_oracle.TapEdge (every digit product and every weighted term of the pseudo-Mersenne accumulation above q_r) with the constants
    +-(t - 1)/2 as plaintexts on a sparse set of pairs of 64 baby x 64 giant steps: giant step 0 holds all 64 baby steps and baby step 0
    sits in all 64 giant steps (both fold points, BS_FOLD_BABY and BS_FOLD_GIANT = 32, are passed twice), the others hold the pairs
    (i, i) and (i, i + 1)"""
    ctx, orc, _ = tg._base(fhe, oracle_mod, name)
    q, n, L = ctx.q, ctx.n, ctx.k - 1
    E = rs.TapEdge(q, n, T)
    klib, korc = [], []
    for b in range(2):
        kc = E.key_coeff(orc, b)
        klib.append(tg._to_lib(fhe, ctx, kc))
        korc.append(ks.key_to_oracle(orc, kc))
    G = 64
    baby = rs.many_elements(n, G)
    giant = [pow(3, 70 + i, 2 * n) for i in range(G)]
    assert len(set(giant)) == G and 1 not in giant
    plains = np.zeros((G, G, n), dtype=np.uint64)
    for i in range(G):
        for j in range(G):
            if i == 0 or j == 0 or j == i or j == (i + 1) % G:
                plains[i, j, 0] = E.weights[j & 1]
    plan = Plan(fhe, ctx, baby, giant, plains, [klib[j & 1] for j in range(G)], [klib[i & 1] for i in range(G)])
    rng = np.random.default_rng(G)
    c0 = np.stack([rng.integers(0, qi, size=n, dtype=np.uint64) for qi in q[:L]])
    host = np.stack([np.stack([c0, E.source()])])
    want = np.stack([ro.rotate_bsgs(orc, host[0], T, baby, giant, plains, [korc[j & 1] for j in range(G)], [korc[i & 1] for i in range(G)])])
    _check_one(fhe, ctx, plan, host, want, "64x64")
    assert tg._unreduced(fhe, ctx.level(L), tdg._out_of_place(fhe, ctx, plan, host)) == 0
    plan.close()


@pytest.mark.parametrize("where", ["final", "inner"])
@pytest.mark.parametrize("name", SMALL)
def test_drop_edges(fhe, oracle_mod, name, where):
    """family D of the key switch (tests/test_gpu_rotdiag.py test_drop_edges): c_1 the constant 1 on residue 0, the BABY key's row 0 holds
    modswitch_oracle.crafted_tile, plaintext "1": A(0) IS the tiles (plus p sigma_g(c_0) on the kept residues of A(0)_0).
    final: the giant step is the identity, the LAST drop sees every prescribed remainder and final residue, and sigma_g(c_0) holds the
           addends that make the result exactly 0 and q_r - 1 -- fhe_rotate_diag_sum_sp's bytes;
    inner: one giant step h != 1: the drop of v(0) sees tile 1; the result is the oracle's"""
    ctx, orc, _ = tg._base(fhe, oracle_mod, name)
    q, n, L = ctx.q, ctx.n, ctx.k - 1
    g = pow(3, n // 8, 2 * n)
    tiles = ks.drop_tiles(q, n)
    kc = ks.drop_key_rows(orc, tiles)
    key, korc = tg._to_lib(fhe, ctx, kc), ks.key_to_oracle(orc, kc)
    unit = ks.unit_source(q, n)
    one = rd.constant(n, 1)[None, None]
    u = np.stack([mo.switch_residues_levels(tiles[pp], q)[L] for pp in range(2)])
    add = ks.final_addends(u, q)
    host = np.stack([go.sigma(add[0], ks.sigma_inverse(n, g), q[:L]), unit])[None]
    A = ro.inner_sums(orc, host[0], T, [g], one, [korc])
    assert np.array_equal(np.stack([orc.ntt_inv(rs._u64(A[0][1][r]), r) for r in range(ctx.k)]), tiles[1]), "A(0)_1 is not the tile"
    if where == "final":
        giant, (hk, hko) = [1], (None, None)
        want = np.stack([ro.rotate_bsgs(orc, host[0], T, [g], giant, one, [korc], [None])])
        assert np.array_equal(want[0], rd.rotate_diag_sum(orc, host[0], T, [g], [one[0, 0]], [korc]))
        for r in range(L):
            assert set(want[0, 0, r, 2::4]) == {0} and set(want[0, 0, r, 3::4]) == {q[r] - 1}
    else:
        giant = [3]
        hk, hko = tg._key(fhe, oracle_mod, name, 3)
        assert np.array_equal(ro._drop1(orc, A[0][1]), u[1]), "v(0) is not the drop of the tile"
        want = np.stack([ro.rotate_bsgs(orc, host[0], T, [g], giant, one, [korc], [hko])])
    plan = Plan(fhe, ctx, [g], giant, one, [key], [hk])
    host = np.concatenate([host, host, host])
    tg._check_sum_forms(fhe, ctx, plan, host, np.concatenate([want, want, want]))
    plan.close()


@pytest.mark.parametrize("name", ["P8192", "P4096"])
def test_larger_transforms(fhe, oracle_mod, name):
    """n = 8192 on the P8192 primes (the 13-stage transform) and n = 4096 on the P4096 primes (the FP64 transforms order their slots in
    their own way: P and both permutation tables come from the context's own transform)"""
    ctx, orc, _ = tg._base(fhe, oracle_mod, name)
    n = ctx.n
    baby, giant = [1, 3], [2 * n - 1, 1]
    rng = np.random.default_rng(n)
    plains = rng.integers(0, T, size=(2, 2, n), dtype=np.uint64)
    plains[1, 1] = 0                                                    # one absent pair
    plan, kb, kg = _plan(fhe, oracle_mod, name, baby, giant, plains)
    host = tg._operands(ctx, [3], seed=5, count=1)
    tg._check_sum_forms(fhe, ctx, plan, host, np.stack([ro.rotate_bsgs(orc, host[0], T, baby, giant, plains, kb, kg)]))
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

    def ones(G2, G1):
        p = np.zeros((G2, G1, n), dtype=np.uint64)
        p[:, :, 0] = 1 + np.arange(G2 * G1).reshape(G2, G1)
        return p

    def create(h=ctx.h, baby=(1, 3), giant=(1, 3), plains=None, kb=(None, key3), kg=(None, key3), G1=None, G2=None, null=()):
        eb, eg = np.array(baby, dtype=np.uint32), np.array(giant, dtype=np.uint32)
        pl = np.ascontiguousarray(ones(max(len(giant), 1), max(len(baby), 1)) if plains is None else plains, dtype=np.uint64)
        pb = (C.c_void_p * max(len(baby), 1))(*[None if k is None else k.data_ptr() for k in kb])
        pg = (C.c_void_p * max(len(giant), 1))(*[None if k is None else k.data_ptr() for k in kg])
        out = C.c_void_p()
        rc = lib.fhe_rotbsgs_plan_create(h, len(baby) if G1 is None else G1, None if "baby" in null else vp(eb), len(giant) if G2 is None else G2,
                                         None if "giant" in null else vp(eg), None if "plains" in null else vp(pl), None if "kb" in null else pb,
                                         None if "kg" in null else pg, None if "out" in null else C.byref(out))
        if rc == 0:
            lib.fhe_rotbsgs_plan_destroy(out)
        return rc

    torch.cuda.synchronize()
    assert create() == 0
    assert create(h=one.h) == -1 and b"at least 2 primes" in lib.fhe_last_error()
    assert create(G1=0) == -1 and b"baby step count" in lib.fhe_last_error()
    assert create(G2=0) == -1 and b"giant step count" in lib.fhe_last_error()
    many = tuple(range(1, 131, 2))
    assert create(baby=many, kb=(key3,) * 65, plains=ones(2, 65)) == -1 and b"baby step count" in lib.fhe_last_error()
    assert create(giant=many, kg=(key3,) * 65, plains=ones(65, 2)) == -1 and b"giant step count" in lib.fhe_last_error()
    for g in (4, 0, 2 * n, 2 * n + 1):
        assert create(baby=(1, g)) == -1 and b"baby Galois element" in lib.fhe_last_error()
        assert create(giant=(1, g)) == -1 and b"giant Galois element" in lib.fhe_last_error()
    assert create(baby=(3, 3), kb=(key3, key3)) == -1 and b"repeated" in lib.fhe_last_error()
    assert create(giant=(3, 3), kg=(key3, key3)) == -1 and b"repeated" in lib.fhe_last_error()
    bad = ones(2, 2)
    bad[1, 1, n - 1] = T
    assert create(plains=bad) == -1 and b"not below t" in lib.fhe_last_error()
    bad = ones(2, 2)
    bad[1] = 0
    assert create(plains=bad) == -1 and b"giant step 1 has no present pair" in lib.fhe_last_error()
    bad = ones(2, 2)
    bad[:, 0] = 0
    assert create(plains=bad) == -1 and b"baby step 0 has no present pair" in lib.fhe_last_error()
    bad = ones(2, 2)
    bad[0, 1] = 0                                                       # an absent pair is no refusal
    assert create(plains=bad) == 0
    assert create(kb=(None, None)) == -1 and b"null key for baby" in lib.fhe_last_error()
    assert create(kg=(None, None)) == -1 and b"null key for giant" in lib.fhe_last_error()
    assert create(h=None) == -1
    for what in ("baby", "giant", "plains", "kb", "kg", "out"):
        assert create(null=(what,)) == -1, what
    assert create(kb=(key3, key3), kg=(key3, key3)) == 0                # the keys of the element 1 are ignored

    plan = Plan(fhe, ctx, [1, 3], [1, 3], ones(2, 2), [None, key3], [None, key3])
    ct = ctx.level(L).random_ct(2)
    out = torch.full((2, 2, L, n), -1, dtype=torch.int64, device=ctx.device)
    p = lambda t: None if t is None else (t if isinstance(t, C.c_void_p) else _p(t))
    scr, nbytes = plan.scratch(2)

    def call(h=plan.h, src=ct, stride=2 * Ln, dst=out, ostride=2 * Ln, count=2, s=scr, sb=nbytes):
        return lib.fhe_rotate_bsgs_sp(h, p(src), stride, p(dst), ostride, count, p(s), sb, None)

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
    assert lib.fhe_rotbsgs_scratch_bytes(None, 2) == 0
    assert lib.fhe_rotbsgs_scratch_bytes(plan.h, 0) == 0 and lib.fhe_rotbsgs_scratch_bytes(plan.h, 5) == 5 * lib.fhe_rotbsgs_scratch_bytes(plan.h, 1)
    torch.cuda.synchronize()
    assert bool((out == -1).all()), "a refused call wrote its output"
    buf = ct.clone()
    assert call(src=buf, dst=buf) == 0                                  # in place is allowed
    torch.cuda.synchronize()
    plan.close()
