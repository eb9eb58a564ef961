"""GPU: the transform kernels (fhe_ntt_forward / fhe_ntt_inverse / fhe_multiply_plain; csrc/ntt_core.h, k_ntt_fwd* / k_ntt_inv* / k_mulplain* of
csrc/fhe_hip.hip, k_poly_f64 of csrc/dct_fused.hip) on operands whose OUTPUTS are prescribed: 0, 1, 2, floor(q/2), floor(q/2) + 1, q - 2, q - 1 in
half (mixed) or all (dense) of the positions, plus structured companions.  Bit for bit against the CPU oracle, every output below q, inputs unwritten.
tests/ntt_craft.py builds the operands; tests/test_ntt_craft_cpu.py proves on its integer models that these outputs reach the kernels' last
steps in lazy form -- and at n = 1024 the arrays run here ARE the arrays analysed there (ntt_craft.crafted_by_model).

Slot order: the library's NTT-form order is internal and its psi need not be the oracle's.  The transform of the monomial X holds n distinct odd
powers of a primitive 2n-th root -- the same set for every psi --, so matching the values of two exact transforms of X gives the permutation
between their slot orders (ntt_craft.slot_permutation, asserted to be a bijection).  Forward outputs are compared ELEMENT BY ELEMENT through it;
inverse inputs are placed through it.

Kernels per base (asserted through fhe_arith_path, printed per case):
  pm-A / pm-B       k_ntt_fwd_pm, k_ntt_inv_pm, k_mulplain_pm <L, 1, PmA | PmB> at every L of DISPATCH_L; class B folds once in the forward transform
  shoup-lazy-A/-B   the same primes with FHE_NTT_NOPM: k_ntt_fwd<L, true> + canon_below_64q, k_ntt_inv<L, true> (ntt_inv_pass4t), k_mulplain<L, true>;
                    at n >= 8192 an even polynomial count takes k_ntt_fwd2 / k_ntt_inv2, an odd one and FHE_NTT_SINGLE the single kernels
  shoup-small       the 36/37-bit P4096 primes at n = 1024: the same lazy kernels where 2^32 / q is large
  shoup-nolazy-61   the largest 61- and 60-bit primes: k_ntt_fwd<L, false>, k_ntt_inv<L, false>, k_mulplain<L, false>
  shoup-nolazy-A    pm-A primes with FHE_NTT_NOPM + FHE_NTT_NOLAZY: the non-lazy transforms; multiply_plain stays k_mulplain<L, true> (its choice
                    depends on the prime width alone)
  shoup-nolazy-33   the two largest 33-bit primes under FHE_DCT_FORCE_U64: below 2^33 the transforms are not lazy (canon_below_64q needs q >= 2^33)
  fp64              P4096 at n = 4096: k_poly_f64 modes 0, 1, 2 with an even count (two polynomials per workgroup) and an odd one
"""
import numpy as np
import pytest

import ntt_craft as nc

pytestmark = pytest.mark.gpu

ALL_N = (1024, 2048, 4096, 8192, 16384)
CASES = ([("pm-A", n) for n in ALL_N] + [("pm-B", n) for n in ALL_N]
         + [(b, n) for b in ("shoup-lazy-A", "shoup-lazy-B") for n in (1024, 4096, 8192, 16384)] + [("shoup-small", 1024)]
         + [(b, n) for b in ("shoup-nolazy-61", "shoup-nolazy-A", "shoup-nolazy-33") for n in (1024, 8192)] + [("fp64", 4096)])
_sides, _crafted, _oracles = {}, {}, {}


class Side:
    """one base at one n: context, oracle, operands, the permutations between the three slot orders (builder, oracle, library)"""

    def __init__(self, fhe, om, name, n):
        import torch
        assert torch.cuda.is_available(), "GPU tests need a HIP device"
        self.fhe, self.name, self.n = fhe, name, n
        self.q, self.t, self.sw, self.cls = nc.base(name, n)[:4]
        self.k = len(self.q)
        self.ctx = fhe.SEALContext(n, self.q, self.t, switches=self.sw or None)
        self.path = fhe._lib.call("fhe_arith_path", self.ctx.h)
        assert self.path & 3 == self.cls, "%s: fhe_arith_path = %d, the kernels named in the docstring need class %d" % (name, self.path, self.cls)
        self.ev = fhe.Evaluator(self.ctx)
        key = (tuple(self.q), n, self.t)
        if key not in _oracles:
            _oracles[key] = om.Oracle(n, self.q, self.t)
        self.orc = orc = _oracles[key]
        if n == 1024:                                          # the arrays the CPU test analysed
            self.cr = nc.crafted_by_model(name, n)
            bfwd = lambda i, a: nc.exact_fwd(a, nc.tables(self.q[i], n))
        else:
            bfwd = lambda i, a: orc.ntt_fwd(np.array(a, dtype=np.uint64), i).tolist()
            if key not in _crafted:
                _crafted[key] = nc.craft(self.q, n, self.t, bfwd, lambda i, s: orc.ntt_inv(np.array(s, dtype=np.uint64), i).tolist())
            self.cr = _crafted[key]
        x = np.zeros((1, self.k, n), dtype=np.uint64)
        x[:, :, 1] = 1
        lib_x = self.fwd(x)[0]
        orc_x = [orc.ntt_fwd(x[0, i], i) for i in range(self.k)]
        bld_x = [bfwd(i, x[0, i].tolist()) for i in range(self.k)]
        self.o2l = [nc.slot_permutation(orc_x[i], lib_x[i]) for i in range(self.k)]
        self.b2l = [nc.slot_permutation(bld_x[i], lib_x[i]) for i in range(self.k)]
        self.b2o = [nc.slot_permutation(bld_x[i], orc_x[i]) for i in range(self.k)]

    def _run(self, fn, a, ev=None):
        """one batch [polys][k][n] through an evaluator call; the input is asserted unwritten"""
        import torch
        d = self.fhe.to_device(np.ascontiguousarray(a), self.ctx.device)
        keep = d.clone()
        out = fn(ev or self.ev, d)
        torch.cuda.synchronize()
        assert torch.equal(d, keep), "the input was written"
        return self.fhe.to_host(out)

    def fwd(self, a, ev=None):
        return self._run(lambda e, d: e.ntt_forward(d), a, ev)

    def inv(self, a, ev=None):
        return self._run(lambda e, d: e.ntt_inverse(d), a, ev)

    def place(self, slots, perm):
        """slots in the builder's order -> the order `perm` leads to"""
        out = np.empty_like(slots)
        for i in range(self.k):
            out[:, i, perm[i]] = slots[:, i, :]
        return out

    def below_q(self, a):
        return all(int(a[:, i].max()) < self.q[i] for i in range(self.k))


def _side(fhe, om, name, n):
    if (name, n) not in _sides:
        _sides[(name, n)] = Side(fhe, om, name, n)
    return _sides[(name, n)]


def _counts(s, total):
    """the whole batch (odd) and the batch without its last polynomial (even): one and two polynomials per workgroup where the kernels pair"""
    assert total % 2 == 1
    return (total, total - 1)


@pytest.mark.parametrize("name,n", CASES)
def test_forward_transform_of_prescribed_slots(fhe, oracle_mod, name, n):
    s = _side(fhe, oracle_mod, name, n)
    cr = s.cr
    print("\n%s n=%d: fhe_arith_path = %d" % (name, n, s.path))
    want = np.stack([np.stack([s.orc.ntt_fwd(cr.F[j, i], i) for i in range(s.k)]) for j in range(len(cr.F))])      # the oracle's slot order
    evs = [s.ev] + ([fhe.Evaluator(fhe.SEALContext(n, s.q, s.t, switches=dict(s.sw, **nc.SINGLE)))] if "lazy-" in name and n >= 8192 else [])
    for ev in evs:
        for cnt in _counts(s, len(cr.F)):
            got = s.fwd(cr.F[:cnt], ev)
            assert s.below_q(got), "an unreduced residue"
            for i in range(s.k):
                bad = np.argwhere(got[:, i, s.o2l[i]] != want[:cnt, i])
                assert bad.size == 0, "prime %d: %d slots differ from the oracle, first (polynomial, oracle slot) %s: got %d, want %d (%s)" % (
                    i, len(bad), bad[0], got[bad[0][0], i, s.o2l[i][bad[0][1]]], want[bad[0][0], i, bad[0][1]], cr.F_names[bad[0][0]])
                assert np.array_equal(got[:, i, s.b2l[i]], cr.F_slots[:cnt, i])         # mixed / dense: the prescribed pattern itself
            assert np.array_equal(s.inv(got, ev), cr.F[:cnt]), "round trip"


@pytest.mark.parametrize("name,n", CASES)
def test_inverse_transform_to_prescribed_coefficients(fhe, oracle_mod, name, n):
    s = _side(fhe, oracle_mod, name, n)
    cr = s.cr
    print("\n%s n=%d: fhe_arith_path = %d" % (name, n, s.path))
    lib_in, orc_in = s.place(cr.I, s.b2l), s.place(cr.I, s.b2o)
    want = np.stack([np.stack([s.orc.ntt_inv(orc_in[j, i], i) for i in range(s.k)]) for j in range(len(cr.I))])
    assert np.array_equal(want, cr.I_out)
    evs = [s.ev] + ([fhe.Evaluator(fhe.SEALContext(n, s.q, s.t, switches=dict(s.sw, **nc.SINGLE)))] if "lazy-" in name and n >= 8192 else [])
    for ev in evs:
        for cnt in _counts(s, len(cr.I)):
            got = s.inv(lib_in[:cnt], ev)
            assert s.below_q(got), "an unreduced residue"
            bad = np.argwhere(got != want[:cnt])
            assert bad.size == 0, "%d coefficients differ from the oracle, first (polynomial, prime, index) %s: got %d, want %d (%s)" % (
                len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])], cr.I_names[bad[0][0]])
            assert np.array_equal(s.fwd(got, ev), lib_in[:cnt]), "round trip"


@pytest.mark.parametrize("name,n", CASES)
def test_multiply_plain_with_prescribed_products_and_prescribed_slots(fhe, oracle_mod, name, n):
    s = _side(fhe, oracle_mod, name, n)
    cr = s.cr
    print("\n%s n=%d: fhe_arith_path = %d" % (name, n, s.path))
    want = s.orc.multiply_plain(cr.M, cr.plain)
    assert np.array_equal(want, cr.M_out)
    pp = fhe.PreparedPlain(s.ctx, cr.plain)
    assert not pp.sparse
    for cnt in _counts(s, len(cr.M)):
        got = s._run(lambda e, d: e.multiply_plain(d, pp), cr.M[:cnt])
        assert s.below_q(got), "an unreduced residue"
        bad = np.argwhere(got != want[:cnt])
        assert bad.size == 0, "%d coefficients differ from the oracle, first (polynomial, prime, index) %s: got %d, want %d (%s)" % (
            len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])], cr.M_names[bad[0][0]])
    f = s.fwd(cr.M)                                          # the operands themselves: their slots (mid: a prescribed pattern) and the round trip
    for i in range(s.k):
        for j, nm in enumerate(cr.M_names):
            if nm.startswith("mid"):
                assert np.array_equal(f[j, i, s.b2l[i]], cr.M_pat[nm][i])
    assert np.array_equal(s.inv(f), cr.M), "round trip"
