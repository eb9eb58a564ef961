"""GPU: the ct x ct product (csrc/behz.hip) on operands that put chosen values under its base conversions, bit for bit against
the CPU oracle.  tests/behz_craft.py builds the operands from a scalar big-integer restatement of the steps;
tests/test_behz_craft_cpu.py proves, in that restatement, that every target is reached:
  lift cases       steps 0/1: every y_i = [m~ c_i (q/q_i)^-1]_{q_i} at 0, 1, q_i - 2, q_i - 1 and on both sides of the 2^28 and 2^29 splits, all
                   y_i at q_i - 1 (the largest column sum) and at 0, the centred Montgomery remainder r at 0, 1, 0x7FFFFFFF, 0x80000000,
                   0x80000001, 0xFFFFFFFF (the centring branch moves the lifted operand by a whole q), and r = 0x80000000 with y_0 = 0
  floor cases      steps 3/4 through a second operand (c, 0), which makes every output coefficient a scalar case of its own: the same
                   points for y_i = [t D (q/q_i)^-1]_{q_i} (c = 1), and z_j = [f_j (B/b_j)^-1]_{b_j} at 0, 1, b_j - 2, b_j - 1 and on both sides
                   of 2^29 under both signs of the floor value v (c = 2^s)
  magnitude cases  every coefficient of every polynomial floor(q/2) or ceil(q/2): |v| within a bit of min(sa, sb) n t q / 4, the bound
                   the choice of auxiliary primes rests on, and alpha_sk ~ -v / B up to 2^40 (test_behz_craft_cpu.py -s prints them)
Every comparison is with Oracle.multiply / Oracle.square (which run on SEAL's 61-bit auxiliary base: the product must not depend
on the base); every output is checked for unreduced residues; every context is asserted through fhe_arith_path to run the kernels
CONTEXTS names, as far as that value can tell (see CONTEXTS).

The z_j targets depend on the auxiliary primes.  The library offers no way to read its primes back, so that they land on the
DEVICE's z_j rests on behz_craft.library_aux restating fhe_behz_build exactly (58 or 61 bits, the descending search, the skipped
q_i, m_sk first).  Should the two drift apart these tests would still pass -- the oracle does not depend on the base -- and silently
stop hitting the z_j points: a change to fhe_behz_build's choice has to be made in library_aux too."""
import ctypes as C

import numpy as np
import pytest

import behz_craft as bc

pytestmark = pytest.mark.gpu

PM_BOTH = 1 | (2 << 2) | 16          # fhe_arith_path: pseudo-Mersenne q-base (class 1), 58-bit auxiliary base (class 2), two-column conversions
# context -> (base of behz_craft.BASES, switches, fhe_arith_path, the kernels of steps 0/1 and 3/4 it runs)
# What the assertion on fhe_arith_path does NOT establish: the value is 0 as soon as FHE_NTT_NOPM is set, so it cannot tell "+NOPM" from
# "+NOPM+AUX61", and it has no bit for FHE_BEHZ_FUSED_PREPARE, so "+FUSED_PREPARE" reads like the default context.  On those three
# contexts the kernels named are what the switches select in csrc/behz.hip, not something these tests can observe: were a switch
# ignored, they would pass unchanged.  The library exposes nothing else to assert on.
CONTEXTS = {
    "SEAL23_4096": ("SEAL23_4096", {}, PM_BOTH, "k_behz_to_bsk_pm<2>, k_behz_floor_back_pm<2>"),
    "P8192": ("P8192", {}, PM_BOTH, "k_behz_to_bsk_pm<4>, k_behz_floor_back_pm<4>"),
    "SEAL23_2048": ("SEAL23_2048", {}, PM_BOTH, "k_behz_to_bsk_pm<1>, k_behz_floor_back_pm<1>: a single prime, B = b_0"),
    "SMALL": ("SMALL", {}, 2 << 2, "k_behz_to_bsk<3, WIDE> (Dot58), k_behz_floor_back<3, WIDE> (128-bit sums) on 58-bit auxiliary primes"),
    "SEAL23_16384": ("SEAL23_16384", {}, PM_BOTH, "k_behz_to_bsk_pm<8>, k_behz_floor_back_pm<8>: a second group of columns (i % PM_GROUP_Y == 0)"),
    "Q4-prime-t": ("Q4-prime-t", {}, PM_BOTH, "the pseudo-Mersenne kernels with t = 65537: constants that are no powers of two"),
    "Q61x5-n1024": ("Q61x5-n1024", {}, 2 << 2, "k_behz_to_bsk<5, 3>, k_behz_floor_back<5, 3>: 61-bit q-primes on 58-bit auxiliary primes, picked with no slack"),
    "Q61x5-n2048": ("Q61x5-n2048", {}, 0, "k_behz_to_bsk<5, 3>, k_behz_floor_back<5, 3> on 61-bit auxiliary primes: one bit past the 58-bit rule"),
}
for _base in ("SEAL23_4096", "P8192"):
    CONTEXTS.update({
        _base + "+NOPM": (_base, {"FHE_NTT_NOPM": 1}, 0, "the WIDE 128-bit / Dot58 kernels on Shoup transforms"),
        _base + "+CHUNK3": (_base, {"FHE_BEHZ_CHUNK3": 1}, 1 | (2 << 2), "k_behz_to_bsk<K, 3>, k_behz_floor_back<K, 3>: a reduction every three terms"),
        _base + "+AUX61": (_base, {"FHE_BEHZ_AUX61": 1}, 1, "the three-term 128-bit kernels on 61-bit auxiliary primes"),
        _base + "+FUSED_PREPARE": (_base, {"FHE_BEHZ_FUSED_PREPARE": 1}, PM_BOTH, "k_behz_prepare_pm: steps 0/1 inside the forward transforms"),
        _base + "+NOPM+AUX61": (_base, {"FHE_NTT_NOPM": 1, "FHE_BEHZ_AUX61": 1}, 0, "the three-term 128-bit kernels, Shoup transforms, 61-bit auxiliary primes"),
    })
BIG_SIZES = ("SMALL", "Q61x5-n1024")            # n = 1024: 12 x 12 (unreduced tensor sums) and 13 x 13 (the reduced schedule)


@pytest.fixture(scope="module")
def setup(fhe, oracle_mod):
    """context name -> dict(ctx, ev, orc, base, aux); oracles and crafted operands are shared by the contexts of a base"""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    per_base, per_ctx = {}, {}

    def get(name):
        if name not in per_ctx:
            base, switches, path, _ = CONTEXTS[name]
            n, q, t = bc.BASES[base]
            if base not in per_base:
                per_base[base] = dict(orc=oracle_mod.Oracle(n, q, t), crafted={})
            ctx = fhe.SEALContext(n, q, t, switches=switches or None)
            got = fhe._lib.call("fhe_arith_path", ctx.h)
            assert got == path, "%s: fhe_arith_path = %d, the docstring's kernels need %d" % (name, got, path)
            per_ctx[name] = dict(per_base[base], ctx=ctx, ev=fhe.Evaluator(ctx), n=n, q=q, t=t, k=len(q), name=name,
                                 aux=bc.library_aux(q, t, n, aux61="FHE_BEHZ_AUX61" in switches))
        return per_ctx[name]
    return get


def _crafted(s, what):
    """the crafted operands of a base, built once (the z_j cases once per auxiliary base)"""
    key = (what, s["aux"]["bits"]) if what.startswith("floor_z") else what
    if key not in s["crafted"]:
        n, q, t = s["n"], s["q"], s["t"]
        s["crafted"][key] = (bc.lift_cases(q, n) if what == "lift" else bc.floor_y_cases(q, t, n) + (1,) if what == "floor_y" else
                             bc.floor_z_cases(q, t, s["aux"], n)[:3] if what == "floor_z" else bc.floor_z_extra_cases(q, t, s["aux"], n)[0])
    return s["crafted"][key]


def _check(fhe, s, got, want, what):
    """got: device batch [count][size][k][n]; want: list of oracle results"""
    import torch
    cnt = torch.zeros(1, dtype=torch.int64, device=got.device)
    fhe._lib.call("fhe_count_unreduced", s["ctx"].h, C.c_void_p(got.data_ptr()), got.numel() // s["n"] // s["k"], C.c_void_p(cnt.data_ptr()), None)
    assert int(cnt.cpu()[0]) == 0, "%s %s: unreduced residues in the output" % (s["name"], what)
    host = fhe.to_host(got)
    assert host.shape[0] == len(want)
    for i, w in enumerate(want):
        if not np.array_equal(host[i], w):
            poly, prime, coef = (int(x[0]) for x in np.nonzero(host[i] != w))
            raise AssertionError("%s %s, pair %d: %d residues differ from the oracle, the first at polynomial %d, prime %d, coefficient %d"
                                 % (s["name"], what, i, int((host[i] != w).sum()), poly, prime, coef))


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_lift_cases(fhe, setup, name):
    """multiply(a, b), multiply(b, a) and square(a): a crafted at steps 0/1, b a random ciphertext"""
    s = setup(name)
    ev, orc = s["ev"], s["orc"]
    a = _crafted(s, "lift")[0]
    b = orc.random_ct(1, seed=4242)[0]
    da, db = fhe.to_device(a[None], s["ctx"].device), fhe.to_device(b[None], s["ctx"].device)
    _check(fhe, s, ev.multiply(da, db), [orc.multiply(a, b)], "lift a x b")
    _check(fhe, s, ev.multiply(db, da), [orc.multiply(b, a)], "lift b x a")
    _check(fhe, s, ev.square(da), [orc.square(a)], "lift square(a)")


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_floor_cases(fhe, setup, name):
    """a batch of two pairs -- (y_i cases, (1, 0)) and (z_j cases, (c, 0)) -- in both orders, and the same through prepared operands;
    under FHE_BEHZ_AUX61 the z_j cases are the ones built for the 61-bit base.  On the single-prime base six more pairs follow: the
    z_0 targets with |v| near b_0, each against a constant of its own"""
    s = setup(name)
    ev, orc = s["ev"], s["orc"]
    pairs = [_crafted(s, "floor_y"), _crafted(s, "floor_z")] + _crafted(s, "floor_z_extra")
    A = np.stack([a for a, _, _ in pairs])
    Cc = np.stack([bc.constant_ct(s["q"], s["n"], c) for _, _, c in pairs])
    dA, dC = fhe.to_device(A, s["ctx"].device), fhe.to_device(Cc, s["ctx"].device)
    want = [orc.multiply(A[i], Cc[i]) for i in range(len(pairs))]
    flip = [orc.multiply(Cc[i], A[i]) for i in range(len(pairs))]
    _check(fhe, s, ev.multiply(dA, dC), want, "floor a x (c, 0)")
    _check(fhe, s, ev.multiply(dC, dA), flip, "floor (c, 0) x a")
    pA, pC = ev.prepare_operand(dA), ev.prepare_operand(dC)
    _check(fhe, s, ev.multiply(pA, dC), want, "floor prepared a x (c, 0)")
    _check(fhe, s, ev.multiply(dA, pC), want, "floor a x prepared (c, 0)")
    _check(fhe, s, ev.multiply(pC, pA), flip, "floor prepared (c, 0) x prepared a")


def _magnitude(fhe, s, sizes):
    ev, orc, dev = s["ev"], s["orc"], s["ctx"].device
    top = max(max(p) for p in sizes)
    lo, hi = bc.magnitude_cases(s["q"], s["n"], top)
    for sa, sb in sizes:
        if sa == sb and sa >= 5:
            _check(fhe, s, ev.square(fhe.to_device(lo[None, :sa], dev)), [orc.square(lo[:sa])], "maximal square(%d)" % sa)
        if (sa, sb) == (5, 5):                              # size 5 runs as a square only
            continue
        for x, y, what in ((lo[:sa], lo[:sb], "floor x floor"), (lo[:sa], hi[:sb], "floor x ceil")):
            got = ev.multiply(fhe.to_device(x[None], dev), fhe.to_device(y[None], dev))
            _check(fhe, s, got, [orc.multiply(x, y)], "maximal %d x %d %s" % (sa, sb, what))


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_magnitude_cases(fhe, setup, name):
    """2 x 2, 3 x 2 and square(5) of operands at floor(q/2) (and ceil(q/2) in the second operand); 2 x 2 only at n = 16384"""
    s = setup(name)
    _magnitude(fhe, s, [(2, 2)] if name == "SEAL23_16384" else [(2, 2), (3, 2), (5, 5)])


@pytest.mark.parametrize("name", BIG_SIZES)
@pytest.mark.parametrize("size", [12, 13])
def test_magnitude_cases_at_the_two_tensor_sum_schedules(fhe, setup, name, size):
    """12 x 12: the largest product whose tensor sums stay unreduced; 13 x 13: the reduced schedule"""
    _magnitude(fhe, setup(name), [(size, size)])


def test_boundary_base_picks_58_bit_primes_with_no_slack_and_61_bit_ones_one_bit_later(fhe, setup):
    """five 61-bit primes, t = 2^14: need = 342 = 57 x 6 at n = 1024 (58-bit auxiliary primes: pseudo-Mersenne class 2 on the auxiliary
    base), 343 at n = 2048 (61-bit ones: no class); the maximal 13 x 13 product at n = 1024 against the big-integer model, which has no
    auxiliary base at all, as well as the C oracle"""
    from oracle.bigint_model import Model
    s, s2 = setup("Q61x5-n1024"), setup("Q61x5-n2048")
    assert bc.aux_need(s["q"], s["t"], 1024) == 342 == 57 * 6 and bc.aux_need(s2["q"], s2["t"], 2048) == 343
    path = lambda x: fhe._lib.call("fhe_arith_path", x["ctx"].h)
    assert (path(s) >> 2) & 3 == 2 and s["aux"]["bits"] == 58
    assert (path(s2) >> 2) & 3 == 0 and s2["aux"]["bits"] == 61
    lo, _ = bc.magnitude_cases(s["q"], s["n"], 13)
    got = s["ev"].multiply(fhe.to_device(lo[None], s["ctx"].device), fhe.to_device(lo[None], s["ctx"].device))
    _check(fhe, s, got, [s["orc"].multiply(lo, lo)], "maximal 13 x 13")
    m = Model(s["n"], s["q"], s["t"])
    H = m.Q // 2
    assert m._behz_lift([H]) == [H]
    sc = bc.Scalar(s["q"], s["t"], s["aux"])
    # the model's product of constant-coefficient operands: D in closed form (its lifts are all H), then its own fast floor
    D = bc.magnitude_D(H, H, 13, 13, s["n"])
    big = np.array(m.to_rns(_model_floor(m, D)), dtype=np.uint64)
    assert np.array_equal(fhe.to_host(got)[0], big)
    assert np.array_equal(sc.floor_polys(D)[0][12], big[12])


def _model_floor(m, D):
    """steps 3/4 of oracle.bigint_model.Model.multiply on given tensor sums: floor(t D / q) as the fast base conversion rounds it"""
    out = []
    for d in D:
        res = []
        for v in d:
            tv = m.t * v
            Y = m._fastbconv_int(lambda qi: tv % qi)
            res.append(((tv - Y) // m.Q) % m.Q)
        out.append(res)
    return out
