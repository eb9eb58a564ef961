"""What tests/decrypt_craft.py's integer model of k_dec_round (csrc/encrypt.hip) proves on the CPU (no GPU, no library).  Run with -s for
the tables (per base: the histogram of j and the noise bit lengths reached).

  pinning     on the whole crafted row of every base the model's plaintext and noise bit length equal the big-integer formula
              m(x) = ((t x + q // 2) // q) % t, noise(x) = |t x - ((t x + q // 2) // q) q|, and no model assertion fires (a < t, the exact
              division through q_i^-1 mod 2^64, sums below 2^(64 (k + 1)))
  coverage    CONDITIONS, not measurements: every j in 0 .. k occurs; delta = 0 (M == j q) and delta = -1 (M == j q - 1) occur; for every
              listed b with 2^b < h the noises 2^b - 1, 2^b, 2^b + 1 occur; m = 0 and m = t - 1 occur
  quiet       every value of the noise family alone among zero phases has the figure |v|.bit_length(), budget q.bit_length() - figure - 1
  variants    deliberately wrong kernels in the model, judged by what the device call RETURNS (plaintexts, one figure per ciphertext):
              `>` for `>=` in big_ge changes the plaintext at delta = 0 in every base and nothing else; the carry without c2 changes
              plaintexts at 61-bit primes and nothing on the 36-bit base; 64 - clz taken from the word before the borrow changes the
              figure of quiet ciphertexts in every base above 66 bits
"""
from collections import Counter

import pytest

import decrypt_craft as dc

IDS = ["%s-k%d-t%d" % c for c in dc.CASES]


@pytest.mark.parametrize("name,k,t", dc.CASES, ids=IDS)
def test_model_equals_the_big_integer_formula_on_the_crafted_row(name, k, t):
    cr = dc.craft(name, k, t)
    assert cr.t < min(cr.q) and len(cr.x) == dc.N and all(0 <= x < cr.Q for x in cr.x)
    for c, (m, bits, j) in enumerate(cr.model):
        assert m == cr.want_plain[c], (c, m, cr.want_plain[c])
        assert bits == cr.want_noise[c].bit_length(), (c, bits, cr.want_noise[c])
    C = cr.C
    for c, x in enumerate(cr.x):                                  # j's own definition: floor((sum_i r_i (q/q_i) + floor(q/2)) / q)
        r = [cr.t * (x % p * ip % p) % p for p, ip in zip(cr.q, C.inv_punct)]
        assert cr.model[c][2] == (sum(ri * P for ri, P in zip(r, C.punct)) + cr.Q // 2) // cr.Q


@pytest.mark.parametrize("name,k,t", dc.CASES, ids=IDS)
def test_coverage_conditions(name, k, t):
    cr = dc.craft(name, k, t)
    Q, h, t = cr.Q, cr.Q // 2, cr.t
    js = Counter(j for _, _, j in cr.model)
    assert set(js) == set(range(k + 1)), "some j in 0 .. k is never computed: %s" % dict(js)
    for d in (0, -1):                                             # (t x + h) mod q == delta: M == j q + delta
        x = cr.x[cr.where[("boundary", d)]]
        assert (t * x + h) % Q == d % Q
    noises = set(cr.want_noise)
    exps = dc.noise_exponents(h)
    assert exps[:4] == [0, 1, 31, 32] and all(64 * w in exps and 64 * w - 1 in exps for w in range(2, (h.bit_length() - 1) // 64 + 1))
    for b in exps:
        assert {(1 << b) - 1, 1 << b, (1 << b) + 1} <= noises, b
        for s in (1, -1):
            for e in (-1, 0, 1):
                assert cr.want_noise[cr.where[("noise", (b, s, e))]] == abs(s * (1 << b) + e)
    assert 0 in noises and cr.want_noise[cr.where[("ends", "h")]] == dc.noise_of(h, Q, t)
    assert 0 in cr.want_plain and t - 1 in cr.want_plain
    assert cr.want_plain[cr.where[("plain", "first t-1")]] == t - 1 == cr.want_plain[cr.where[("plain", "last t-1")]]
    assert cr.want_plain[cr.where[("plain", "last 0")]] == 0 and cr.want_plain[cr.where[("plain", "first 1")]] == 1 % t
    assert cr.want_plain[cr.where[("ends", "q-1")]] == (t - 1 if h < t else 0)      # t x + h = t q - (t - h): the quotient t wraps to 0
    lengths = sorted(set(v.bit_length() for v in cr.want_noise))
    print("\n%s k=%d t=%d (q: %d bits): j histogram %s; noise bit lengths %s" % (name, k, t, Q.bit_length(), dict(sorted(js.items())), lengths))


@pytest.mark.parametrize("name,k,t", dc.CASES, ids=IDS)
def test_quiet_ciphertexts_carry_one_noise_length_each(name, k, t):
    """every value of the noise family alone among zero phases: the model's figure of that ciphertext is |v|.bit_length(), the phase 0
    gives (0, 0 bits), and the budget is q.bit_length() - figure - 1, positive below the top bit length"""
    cr = dc.craft(name, k, t)
    h, qbits = cr.Q // 2, cr.Q.bit_length()
    assert dc.round_model([0] * k, cr.C) == (0, 0, 0)
    want = set()
    for b in dc.noise_exponents(h):
        want |= {(1 << b) - 1, 1 << b, (1 << b) + 1}
    assert want <= {abs(v) for _, v, _ in cr.quiet} and {h, -h} <= {v for _, v, _ in cr.quiet}
    for lab, v, pos in cr.quiet:
        x = cr.with_noise(v)
        m, bits, _ = dc.round_model([x % p for p in cr.q], cr.C)
        assert dc.noise_of(x, cr.Q, t) == abs(v) and bits == abs(v).bit_length() and m == dc.plain_of(x, cr.Q, t), lab
        assert dc.budget_of(bits, cr.Q) == qbits - bits - 1 >= 0, lab                # |v| <= h < 2^(qbits - 1): zero only in the top bit lengths
    print("\n%s k=%d t=%d: %d quiet ciphertexts, figures %s" % (name, k, t, len(cr.quiet), sorted({abs(v).bit_length() for _, v, _ in cr.quiet})))


def _observed(cr, **variant):
    """what fhe_decrypt_batch RETURNS for the tests' ciphertexts under a variant of the kernel: the plaintexts and the ONE figure of the
    crafted row, and (plaintext of the loud coefficient, figure) of every quiet ciphertext -- a coefficient's own bit length is no output"""
    row = [dc.round_model([x % p for p in cr.q], cr.C, **variant) for x in cr.x]
    assert dc.round_model([0] * cr.k, cr.C, **variant) == (0, 0, 0)
    quiet = {lab: dc.round_model([cr.with_noise(v) % p for p in cr.q], cr.C, **variant)[:2] for lab, v, _ in cr.quiet}
    return [m for m, _, _ in row], max(b for _, b, _ in row), quiet


def _diff(cr, **variant):
    """(coefficients of the crafted row whose PLAINTEXT changes, (figure, figure under the variant) of the row, {quiet label: (right, wrong)})"""
    (p0, f0, q0), (p1, f1, q1) = _observed(cr), _observed(cr, **variant)
    return [c for c in range(cr.n) if p0[c] != p1[c]], (f0, f1), {lab: (q0[lab], q1[lab]) for lab in q0 if q0[lab] != q1[lab]}


def test_deliberately_wrong_kernels_change_what_the_device_tests_compare():
    """Observables only: plaintexts, and one figure per ciphertext.
    `>` for `>=`: in EVERY base the plaintext of the delta = 0 coefficient of the crafted row (M == j q: j one short) and of the quiet
    ciphertext -h (the same phase), nothing else.
    No c2: plaintexts of the W61 k = 8 row (61-bit r_i against 64-bit words of q/q_i wrap s1 + carry in about one step of 16); nothing on
    the 36-bit base.
    clz of the word before the borrow: in every base above 66 bits the figure of quiet ciphertexts whose top difference word is a
    power of two above a borrow (noise 2^b - 1 or 2^b + 1 at b >= 64) -- while the figure of the crafted ROW, owned by the filler, need not move."""
    for name, k, t in dc.CASES:
        cr = dc.craft(name, k, t)
        plains, figure, quiet = _diff(cr, gt=True)
        assert plains == [cr.where[("boundary", 0)]] and figure[0] == figure[1] and set(quiet) == {"-h"}, (name, k, t)
        (m0, b0), (m1, b1) = quiet["-h"]
        assert m1 == (m0 - 1) % cr.t
        plains, figure, quiet = _diff(cr, clz_prev=True)
        assert not plains, "the noise figure does not touch the plaintext"
        if cr.Q.bit_length() > 66:
            assert quiet and all(right[1] + 1 == wrong[1] and right[0] == wrong[0] for right, wrong in quiet.values()), (name, k, t)
            print("\nclz before the borrow, %s k=%d t=%d: row figure %d -> %d; quiet figures %s" % (
                name, k, t, figure[0], figure[1], sorted((lab, right[1], wrong[1]) for lab, (right, wrong) in quiet.items() if lab not in ("h", "-h"))[:6]))
    cr = dc.craft("Q4", 3, 65537)
    c = cr.where[("boundary", 0)]
    print("`>` for `>=`, Q4 k=3 t=65537: plaintext of coefficient %d (delta = 0) %d -> %d" % (c, cr.want_plain[c], _observed(cr, gt=True)[0][c]))
    cr = dc.craft("W61", 8, (1 << 60) - 1)
    plains, figure, quiet = _diff(cr, drop_c2=True)
    assert plains, "dropping c2 changes no plaintext at 61-bit primes"
    wrong = _observed(cr, drop_c2=True)[0]
    print("no c2, W61 k=8 t=2^60-1: %d plaintexts of the row change, first: coefficient %d, %d -> %d; row figure %d -> %d; %d quiet ciphertexts change" % (
        len(plains), plains[0], cr.want_plain[plains[0]], wrong[plains[0]], figure[0], figure[1], len(quiet)))
    assert _diff(dc.craft("Q3", 2, 12289), drop_c2=True) == ([], (71, 71), {})
