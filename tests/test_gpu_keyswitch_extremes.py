"""GPU: the key switch (fhe_relinearize_poly / fhe_relinearize_n / fhe_apply_galois; csrc/behz.hip k_relin_*, csrc/galois.hip k_galois_*)
on operands built to sit on the bounds its lazy arithmetic is written for, bit for bit against the CPU oracle.  tests/keyswitch_craft.py
builds the operands from a one-slot integer restatement; tests/test_keyswitch_craft_cpu.py proves, in that restatement, that the
targets are reached:
  family D   real keys; every coefficient of the source carries a chosen digit pattern (0, 1, 2^dbc - 2, 2^dbc - 1, q_ii - 1, q_ii, q_ii + 1
             where the digit reaches them, the top digit's maximum, one above what a narrower prime holds), whole polynomials carry the
             digit maximum; at every decomposition bit count of keyswitch_craft.dbc_rule -- the `wide` boundary of every prime width, 1,
             60, the longest lazy sum and the first dbc on the general path, every dbc at which the primes differ in digit count
  family U   constant source polynomials and keys crafted per slot: every lazy product of every 20-term sum at or above q_ii, every slot
             of the inverse transform entered above q_ii; the key q_ii - 1 everywhere; the key 0 in polynomial 1
  both       c0 / c1 at 0, q - 1, and the values that make the final sum exactly q and q - 1
Every call is checked for unreduced residues, for an untouched input, and in place against out of place.

The kernels a base runs (printed per case with fhe_arith_path and the restated gate k x digits x powers <= 20):
  A, B          gate holds: k_relin_fwd_pm / k_galois_fwd_pm<L, PmA | PmB>, k_relin_accum_pm, k_relin_inv_add_pm / k_galois_inv_add_pm
                (+FHE_RELIN_FUSED: k_relin_accum_inv_add_pm; +FHE_GALOIS_STAGED: k_galois_stage; +FHE_GALOIS_GATHER_LDS: the LDS gather);
                gate fails (small dbc): the general kernels below on the pseudo-Mersenne transforms
  A-nopm        k_relin_digits / k_galois_digits, k_relin_accum, k_relin_add / k_galois_add, Shoup transforms
  P4096-n1024   the same kernels on the 36/37-bit primes;  P4096 (n = 4096): with the exact-FP64 transforms
"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import galois_oracle as go
import keyswitch_craft as kc

pytestmark = pytest.mark.gpu

VARIANTS = {"fused": {"FHE_RELIN_FUSED": 1}, "staged": {"FHE_GALOIS_STAGED": 1}, "gather": {"FHE_GALOIS_GATHER_LDS": 1}, "steps+fused": {"FHE_RELIN_STEPS": 1, "FHE_RELIN_FUSED": 1}}
_cache = {}
_pool = ThreadPoolExecutor(max_workers=8)          # the oracle's calls release the interpreter lock: one ciphertext per thread


def _wide_boundary(q):
    return {d for p in q for d in (p.bit_length() - 1, p.bit_length())}


def _d_cases():
    out = []
    for name, (n, q, sw, cls) in kc.BASES.items():
        for dbc in sorted(set(kc.dbc_rule(q)) | ({30} if cls else set())):
            out.append((name, dbc))
    return out


class Side:
    """one base at one n: the default context, its variants, the oracle, a secret key"""

    def __init__(self, fhe, om, name, n):
        import torch
        assert torch.cuda.is_available(), "GPU tests need a HIP device"
        self.fhe, self.name, self.n = fhe, name, n
        self.q, self.sw, self.cls = kc.base_at(name, n)
        self.k = len(self.q)
        self.ctx = fhe.SEALContext(n, self.q, kc.T_PLAIN, switches=self.sw or None)
        self.path = fhe._lib.call("fhe_arith_path", self.ctx.h)
        assert self.path & 3 == self.cls, "%s: fhe_arith_path = %d, the kernels named in the docstring need class %d" % (name, self.path, self.cls)
        self.orc = om.Oracle(n, self.q, kc.T_PLAIN)
        self.ev = fhe.Evaluator(self.ctx)
        self.sk = self.orc.keygen(7)[0]
        self._variants, self.keys = {}, {}

    def variant(self, which):
        if which not in self._variants:
            self._variants[which] = self.fhe.SEALContext(self.n, self.q, kc.T_PLAIN, switches=dict(self.sw, **VARIANTS[which]))
        return self._variants[which]

    def pm(self, dbc, npow=1):
        """the restated gate's verdict: do the pseudo-Mersenne key-switch kernels run"""
        return bool(self.cls) and kc.gate(self.k, kc.digits(self.q, dbc), npow)

    def device_key(self, key):
        """oracle NTT form -> the oracle's ntt_inv -> the library's ntt_forward: each side keeps its own slot order"""
        flat = key.reshape(-1, self.k, self.n)
        coeff = np.stack(list(_pool.map(lambda p: np.stack([self.orc.ntt_inv(p[i], i) for i in range(self.k)]), flat))).reshape(key.shape)
        return self.ev.ntt_forward(self.fhe.to_device(coeff, self.ctx.device)).contiguous()

    def real_key(self, dbc, what):
        """what: "relin" -> keys for s^2 and s^3 [2][k][nd][2][k][n]; a Galois element's index -> one key set from the oracle's generator (the key
        switch does not know what its key is a key for)"""
        if (dbc, what) not in self.keys:
            key = self.orc.evk_gen_powers(self.sk, dbc=dbc, count=2) if what == "relin" else self.orc.evk_gen(self.sk, dbc=dbc, seed=100 + what)
            self.keys[(dbc, what)] = (key, self.device_key(key))
        return self.keys[(dbc, what)]


def _side(fhe, om, name, n=None):
    n = kc.BASES[name][0] if n is None else n
    if (name, n) not in _cache:
        _cache[(name, n)] = Side(fhe, om, name, n)
    return _cache[(name, n)]


def _p(t):
    return C.c_void_p(t.data_ptr())


def _scratch(s, nbytes):
    import torch
    return torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=s.ctx.device)


def _call_relin(s, ctx, ct, src_poly, evk, dbc, in_place=False, n_size=None, keeps_input=True):
    """fhe_relinearize_poly (n_size None) or fhe_relinearize_n on a batch [count][size][k][n]; in place: the result lands on c0 / c1 of a copy"""
    import torch
    L = s.fhe._lib.load()
    count, size, kn = ct.shape[0], ct.shape[1], s.k * s.n
    work = ct.clone()
    out = work if in_place else torch.empty((count, 2, s.k, s.n), dtype=torch.int64, device=ct.device)
    ostride = size * kn if in_place else 2 * kn
    if n_size is None:
        nbytes = L.fhe_relinearize_scratch_bytes(ctx.h, dbc, count)
        s.fhe._lib.call("fhe_relinearize_poly", ctx.h, _p(work), size * kn, src_poly, _p(out), ostride, count, _p(evk), dbc, _p(_scratch(s, nbytes)), nbytes, None)
    else:
        nbytes = L.fhe_relinearize_n_scratch_bytes(ctx.h, n_size, dbc, count)
        s.fhe._lib.call("fhe_relinearize_n", ctx.h, _p(work), n_size, size * kn, _p(out), ostride, count, _p(evk), dbc, _p(_scratch(s, nbytes)), nbytes, None)
    torch.cuda.synchronize()
    if in_place:
        return out[:, :2].contiguous()
    # a single pass never writes its input; fhe_relinearize_n runs all passes but the last in place on c0 / c1, by contract
    assert torch.equal(work if keeps_input else work[:, 2:], ct if keeps_input else ct[:, 2:]), "the input was written"
    return out


def _call_galois(s, ctx, ct, g, evk, dbc, in_place=False):
    import torch
    L = s.fhe._lib.load()
    count, kn = ct.shape[0], s.k * s.n
    src = ct.clone()
    out = src if in_place else torch.empty_like(ct)
    nbytes = L.fhe_apply_galois_scratch_bytes(ctx.h, dbc, count)
    s.fhe._lib.call("fhe_apply_galois", ctx.h, _p(src), 2 * kn, _p(out), 2 * kn, count, g, _p(evk), dbc, _p(_scratch(s, nbytes)), nbytes, None)
    torch.cuda.synchronize()
    if not in_place:
        assert torch.equal(src, ct), "the input was written"
    return out


def _check(s, got, want, what):
    """got: device [count][2][k][n]; want: the oracle's results"""
    import torch
    cnt = torch.zeros(1, dtype=torch.int64, device=got.device)
    s.fhe._lib.call("fhe_count_unreduced", s.ctx.h, _p(got), got.numel() // s.n // s.k, _p(cnt), None)
    assert int(cnt.cpu()[0]) == 0, "%s %s: unreduced residues in the output" % (s.name, what)
    host = s.fhe.to_host(got)
    assert host.shape[0] == len(want)
    for i, w in enumerate(want):
        if not np.array_equal(host[i], w):
            poly, prime, coef = (int(x[0]) for x in np.nonzero(host[i] != w))
            raise AssertionError("%s %s, ciphertext %d: %d residues differ from the oracle, the first at polynomial %d, prime %d, coefficient %d (got %d, oracle %d)"
                                 % (s.name, what, i, int((host[i] != w).sum()), poly, prime, coef, int(host[i][poly, prime, coef]), int(w[poly, prime, coef])))


def _orc_poly(orc, ct, src_poly, key, dbc):
    out = np.ascontiguousarray(ct).copy()
    key = np.ascontiguousarray(key)
    orc.L.fo_relinearize_poly(orc.h, out.ctypes.data_as(C.c_void_p), src_poly, key.ctypes.data_as(C.c_void_p), dbc)
    return out[:2].copy()


def _relin_everywhere(s, dev, src_poly, dkey, dbc, want, what, variants=(), n_size=None):
    """the default context out of place and in place against the oracle; every variant context must give the same bits"""
    import torch
    one_pass = n_size is None or len(kc.passes(n_size, s.k, kc.digits(s.q, dbc), bool(s.cls))) == 1
    got = _call_relin(s, s.ctx, dev, src_poly, dkey, dbc, n_size=n_size, keeps_input=one_pass)
    _check(s, got, want, what)
    assert torch.equal(_call_relin(s, s.ctx, dev, src_poly, dkey, dbc, in_place=True, n_size=n_size), got), "%s %s: in place differs" % (s.name, what)
    for v in variants:
        assert torch.equal(_call_relin(s, s.variant(v), dev, src_poly, dkey, dbc, n_size=n_size, keeps_input=n_size is None), got), "%s %s: FHE switches %r give other bits" % (s.name, what, VARIANTS[v])
        assert torch.equal(_call_relin(s, s.variant(v), dev, src_poly, dkey, dbc, in_place=True, n_size=n_size), got), "%s %s: %r in place differs" % (s.name, what, VARIANTS[v])
    return got


def _galois_everywhere(s, dev, g, dkey, dbc, want, what, variants=()):
    import torch
    got = _call_galois(s, s.ctx, dev, g, dkey, dbc)
    _check(s, got, want, what)
    assert torch.equal(_call_galois(s, s.ctx, dev, g, dkey, dbc, in_place=True), got), "%s %s: in place differs" % (s.name, what)
    for v in variants:
        assert torch.equal(_call_galois(s, s.variant(v), dev, g, dkey, dbc), got), "%s %s: FHE switches %r give other bits" % (s.name, what, VARIANTS[v])
        assert torch.equal(_call_galois(s, s.variant(v), dev, g, dkey, dbc, in_place=True), got), "%s %s: %r in place differs" % (s.name, what, VARIANTS[v])
    return got


def _report(s, family, dbc, npow=1, extra=""):
    nd = kc.digits(s.q, dbc)
    print("\n[keyswitch %s %s n=%d k=%d dbc=%d digits=%d powers=%d] arith path %d, restated gate (k x digits x powers = %d <= %d): %s%s"
          % (family, s.name, s.n, s.k, dbc, nd, npow, s.path, s.k * nd * npow, kc.MAX_TERMS,
             "pseudo-Mersenne key-switch kernels" if s.pm(dbc, npow) else "general kernels", extra))


# ---- family D -----------------------------------------------------------------------------------------------------------------------
def _d_sources(s, dbc):
    if ("D", dbc) not in s.keys:
        s.keys[("D", dbc)] = kc.digit_sources(s.q, s.n, dbc)[0]
    return s.keys[("D", dbc)]


@pytest.mark.parametrize("op", ["relin", 0, 1, 2, 3])
@pytest.mark.parametrize("name,dbc", _d_cases())
def test_digit_edges(fhe, oracle_mod, name, dbc, op):
    """op "relin": fhe_relinearize_poly with source polynomial 2 and 3 of a size-4 batch (polynomial 3 holds the patterns in reversed coefficient
    order); op 0 .. 3: fhe_apply_galois with that element of galois_oracle.elements, on the source whose image under sigma_g is the pattern
    and on the direct form, whose stored values q_i - pattern sit where the kernel negates"""
    s = _side(fhe, oracle_mod, name)
    orc, q, n = s.orc, s.q, s.n
    src = _d_sources(s, dbc)
    cnt = src.shape[0]
    variants = ("fused", "staged", "gather") if s.cls and dbc in _wide_boundary(q) | {30} else ()
    _report(s, "D", dbc, extra="; %d ciphertexts, variants %r" % (cnt, variants))
    if op == "relin":
        keys, dkeys = s.real_key(dbc, "relin")
        ct = np.zeros((cnt, 4, s.k, n), dtype=np.uint64)
        ct[:, 2], ct[:, 3] = src, src[:, :, ::-1]
        for p in (2, 3):
            acc = list(_pool.map(lambda c: _orc_poly(orc, c, p, keys[p - 2], dbc), ct))
            full = ct.copy()
            full[:, :2] = np.stack([kc.final_addends(a, q) for a in acc])
            want = list(_pool.map(lambda c: _orc_poly(orc, c, p, keys[p - 2], dbc), full))
            _relin_everywhere(s, fhe.to_device(full, s.ctx.device), p, dkeys[p - 2].contiguous(), dbc, want, "D dbc %d source polynomial %d" % (dbc, p), variants)
        return
    g = go.elements(n)[op][0]
    ginv = pow(g, -1, 2 * n)
    key, dkey = s.real_key(dbc, op)
    for form, c1 in (("image", go.sigma(src, ginv, q)), ("direct", kc.direct_form(src, g, q))):
        ct = np.zeros((cnt, 2, s.k, n), dtype=np.uint64)
        ct[:, 1] = c1
        acc = list(_pool.map(lambda c: go.apply_galois(orc, c, g, key, dbc), ct))
        ct[:, 0] = go.sigma(np.stack([kc.final_addends(a, q)[0] for a in acc]), ginv, q)
        want = list(_pool.map(lambda c: go.apply_galois(orc, c, g, key, dbc), ct))
        _galois_everywhere(s, fhe.to_device(ct, s.ctx.device), g, dkey, dbc, want, "D dbc %d g %d %s form" % (dbc, g, form), variants)


# ---- family U -----------------------------------------------------------------------------------------------------------------------
def _u_dbcs(name):
    """dbc 60, the dbc of the longest sum (20 terms on the pseudo-Mersenne bases, at most 24 on the general-path controls), one in between"""
    q = kc.BASES[name][1]
    edge = kc.twenty_term_dbc(q) if kc.BASES[name][3] else kc.control_dbc(q)
    return [60, {"A": 27, "B": 30, "A-nopm": 27}.get(name, 18), edge]


def _uniform(s, dbc, npow):
    if ("U", dbc, npow) not in s.keys:
        s.keys[("U", dbc, npow)] = kc.Uniform(s.q, s.n, dbc, npow, pm=s.pm(dbc, 1))
    return s.keys[("U", dbc, npow)]


def _u_key(s, u, kind):
    if ("Ukey", u.dbc, u.npow, kind) not in s.keys:
        s.keys[("Ukey", u.dbc, u.npow, kind)] = s.device_key(u.key(kind))
    return u.key(kind), s.keys[("Ukey", u.dbc, u.npow, kind)]


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("name", list(kc.BASES))
def test_uniform_sums_one_key_switch(fhe, oracle_mod, name, which):
    """fhe_relinearize_poly and fhe_apply_galois (fused and staged) of family U with its three keys; FHE_RELIN_FUSED must give the same bits"""
    s = _side(fhe, oracle_mod, name)
    dbc = _u_dbcs(name)[which]
    u = _uniform(s, dbc, 1)
    orc, q, n = s.orc, s.q, s.n
    _report(s, "U", dbc, extra="; %d-term sums" % (s.k * u.nd))
    for kind in kc.Uniform.KINDS:
        key, dkey = _u_key(s, u, kind)
        c01 = kc.final_addends(orc.relinearize(u.ct(3), key[0], dbc), q)
        ct = np.stack([u.ct(3, c01), u.ct(3)])
        want = [orc.relinearize(c, key[0], dbc) for c in ct]
        if kind == "zero1":
            assert np.array_equal(want[0][1], c01[1]) and not want[1][1].any()
        _relin_everywhere(s, fhe.to_device(ct, s.ctx.device), 2, dkey[0].contiguous(), dbc, want, "U %s dbc %d" % (kind, dbc), ("fused",) if s.cls else ())
        for g, _, _ in go.elements(n):
            ct2 = np.zeros((1, 2, s.k, n), dtype=np.uint64)
            ct2[0, 1, :, 0] = u.src
            ct2[0, 0] = go.sigma(c01[0], pow(g, -1, 2 * n), q)
            _galois_everywhere(s, fhe.to_device(ct2, s.ctx.device), g, dkey[0].contiguous(), dbc, [go.apply_galois(orc, ct2[0], g, key[0], dbc)],
                               "U %s dbc %d g %d" % (kind, dbc, g), ("staged",))


U_SIZES = [("A", 4), ("A", 7), ("A", 8), ("B", 4), ("B", 12), ("B", 13), ("A-nopm", 8), ("P4096-n1024", 10), ("P4096", 10)]


def _relin_n_case(fhe, s, size, kinds=("crafted",)):
    orc, q = s.orc, s.q
    u = _uniform(s, 60, size - 2)
    groups = kc.passes(size, s.k, u.nd, bool(s.cls))
    _report(s, "U", 60, size - 2, extra="; size %d, passes over the polynomials %r" % (size, groups))
    for kind in kinds:
        key, dkey = _u_key(s, u, kind)
        c01 = kc.final_addends(orc.relinearize_n(u.ct(size), key, 60), q)
        ct = np.stack([u.ct(size, c01), u.ct(size)])
        want = [orc.relinearize_n(c, key, 60) for c in ct]
        _relin_everywhere(s, fhe.to_device(ct, s.ctx.device), 0, dkey, 60, want, "U %s size %d" % (kind, size), ("steps+fused", "fused") if s.cls else ("steps+fused",), n_size=size)
    return groups


@pytest.mark.parametrize("name,size", U_SIZES)
def test_uniform_sums_relinearize_n(fhe, oracle_mod, name, size):
    """fhe_relinearize_n at dbc 60: 20 terms in one pass at sizes 7 (class A) and 12 (class B), two passes one size above; the general-path
    bases with 24 canonical terms as the control; the default context against FHE_RELIN_STEPS=1 + FHE_RELIN_FUSED=1 (single key switches
    through k_relin_accum_inv_add_pm) and against FHE_RELIN_FUSED=1 alone (all 20 terms of a pass inside that kernel)"""
    s = _side(fhe, oracle_mod, name)
    groups = _relin_n_case(fhe, s, size, kc.Uniform.KINDS if size in (7, 12) else ("crafted",))
    if (name, size) in (("A", 8), ("B", 13)):
        assert len(groups) == 2 and groups[0][1] - groups[0][0] + 1 == size - 3
    elif s.cls:
        assert groups == [(2, size - 1)]
    else:
        assert len(groups) == size - 2 and s.k * (size - 2) <= kc.CONTROL_TERMS


@pytest.mark.parametrize("name,n", [(name, n) for name in kc.SIZES_N for n in kc.SIZES_N[name]])
def test_uniform_sums_at_every_transform_size(fhe, oracle_mod, name, n):
    """the 20-term size through fhe_relinearize_n at every n the key switch instantiates (the static range plans of the inverse transform
    differ by size), and one key switch of it through fhe_apply_galois"""
    s = _side(fhe, oracle_mod, name, n)
    size = {"A": 7, "B": 12}[name]
    assert _relin_n_case(fhe, s, size) == [(2, size - 1)]
    u = _uniform(s, 60, 1)
    key, dkey = _u_key(s, u, "crafted")
    g = go.elements(n)[3][0]
    ct2 = np.zeros((1, 2, s.k, n), dtype=np.uint64)
    ct2[0, 1, :, 0] = u.src
    ct2[0, 0, :, :] = np.array(s.q, dtype=np.uint64)[:, None] - np.uint64(1)
    _galois_everywhere(s, fhe.to_device(ct2, s.ctx.device), g, dkey[0].contiguous(), 60, [go.apply_galois(s.orc, ct2[0], g, key[0], 60)], "U n %d g %d" % (n, g), ("staged", "gather"))


def test_strided_batch_keeps_its_gaps(fhe, oracle_mod):
    """three ciphertexts of family U (size 7, 20-term sums) with gaps on both sides through fhe_relinearize_n, and their first key switch
    through fhe_relinearize_poly and fhe_apply_galois: the gaps stay -1, the input stays as it was"""
    import torch
    s = _side(fhe, oracle_mod, "A")
    orc, q, n, k = s.orc, s.q, s.n, s.k
    kn, size, count = k * n, 7, 3
    u = _uniform(s, 60, size - 2)
    key, dkey = _u_key(s, u, "crafted")
    c01 = kc.final_addends(orc.relinearize_n(u.ct(size), key, 60), q)
    top = np.broadcast_to(np.array(q, dtype=np.uint64)[None, :, None] - np.uint64(1), (2, k, n))
    cts = np.stack([u.ct(size, c01), u.ct(size), u.ct(size, top)])
    L = fhe._lib.load()
    si, so = size * kn + 3 * n, 2 * kn + 5 * n
    src = torch.full((count, si), -1, dtype=torch.int64, device=s.ctx.device)
    src[:, :size * kn] = fhe.to_device(cts, s.ctx.device).reshape(count, size * kn)
    before = src.clone()
    _report(s, "U", 60, size - 2, extra="; strided batch of %d" % count)

    def run(fn, call):
        dst = torch.full((count, so), -1, dtype=torch.int64, device=s.ctx.device)
        call(dst)
        torch.cuda.synchronize()
        assert torch.equal(src, before), fn + ": the input or its gaps were written"
        assert bool((dst[:, 2 * kn:] == -1).all()), fn + ": the output's gaps were written"
        return dst[:, :2 * kn].reshape(count, 2, k, n).contiguous()

    nb = max(L.fhe_relinearize_n_scratch_bytes(s.ctx.h, size, 60, count), L.fhe_apply_galois_scratch_bytes(s.ctx.h, 60, count))
    scr, key0 = _scratch(s, nb), dkey[0].contiguous()
    got = run("fhe_relinearize_n", lambda dst: fhe._lib.call("fhe_relinearize_n", s.ctx.h, _p(src), size, si, _p(dst), so, count, _p(dkey), 60, _p(scr), nb, None))
    _check(s, got, [orc.relinearize_n(c, key, 60) for c in cts], "strided fhe_relinearize_n")
    got = run("fhe_relinearize_poly", lambda dst: fhe._lib.call("fhe_relinearize_poly", s.ctx.h, _p(src), si, 2, _p(dst), so, count, _p(key0), 60, _p(scr), nb, None))
    _check(s, got, [orc.relinearize(c[:3], key[0], 60) for c in cts], "strided fhe_relinearize_poly")
    g = go.elements(n)[0][0]
    got = run("fhe_apply_galois", lambda dst: fhe._lib.call("fhe_apply_galois", s.ctx.h, _p(src), si, _p(dst), so, count, g, _p(key0), 60, _p(scr), nb, None))
    _check(s, got, [go.apply_galois(orc, c[:2], g, key[0], 60) for c in cts], "strided fhe_apply_galois")
