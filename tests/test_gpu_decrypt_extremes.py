"""GPU: fhe_decrypt_batch (csrc/encrypt.hip: k_dec_horner, k_dec_round<K>) driven to its arithmetic edges, bit for bit against Python big
integers: m(x) = ((t x + q // 2) // q) % t and the bit length of |t x - ((t x + q // 2) // q) q| (tests/decrypt_craft.py; the coverage
conditions of the crafted rows are proved on the CPU by tests/test_decrypt_craft_cpu.py -- the rows run here ARE those rows).

  rounding      one case per (base, k, t) of decrypt_craft.CASES: every k_dec_round<K>, K = 1 .. 8, primes of 33 to 61 bits, t from 257 to
                2^60 - 1.  A size-2 ciphertext (c_0, 0) has phase c_0 under every key: the crafted row, its reverse and a random row
  noise length  the call reports ONE figure per ciphertext, a maximum over its coefficients, and in the crafted row the random filler (noise
                about q/2) owns it: every value of the noise family (2^b - 1, 2^b, 2^b + 1 from both signs at every word boundary, and +-h)
                ALONE in a ciphertext of zero phases, per (base, k, t): figure |v|.bit_length(), budget qbits - figure - 1
  maximum       the noise figure is a per-ciphertext maximum folded by shuffles and one atomicMax per wave: ONE loud coefficient (first
                lane of the first wave, last lane of the last, a lane of a middle wave) between silent neighbours
  Horner        the secret key as a CONSTANT per prime (a constant polynomial transforms to that constant in every slot of any slot
                order): s = -1, 1, floor(q_i/2) + 1; sizes 2, 3, 5, FHE_MAX_POLYS; coefficients all q_i - 1, only the last polynomial, random
  grid strides  count n > 65535 * 256 and count k > 32768: both grid-stride loops take a second trip
  refusals      FHE_ERR_PARAM with the output untouched
"""
import ctypes as C
import random
import re

import numpy as np
import pytest

import decrypt_craft as dc

pytestmark = pytest.mark.gpu
assert {k for _, k, _ in dc.CASES} == set(range(1, 9))          # every k_dec_round<K> instantiation


def _header(fhe, name):
    """a #define of include/fhe_hip.h"""
    m = re.search(r"^#define %s \(?(-?\d+)\)?" % name, open(fhe.HEADER_PATH).read(), re.M)
    return int(m.group(1))


SENTINEL = 0x5A5A5A5A5A5A5A5A
_sides = {}


class Side:
    def __init__(self, fhe, name, k, t):
        self.cr = cr = dc.craft(name, k, t)
        self.ctx = fhe.SEALContext(cr.n, cr.q, cr.t)
        self.kg = fhe.KeyGenerator(self.ctx, seed=41)
        self.dec = fhe.Decryptor(self.ctx, self.kg.secret_key())
        self.qbits = int(fhe._lib.load().fhe_ctx_modulus_bits(self.ctx.h))
        assert self.qbits == cr.Q.bit_length()
        assert int(fhe._lib.load().fhe_ctx_k(self.ctx.h)) == k


def _side(fhe, name, k, t):
    if (name, k, t) not in _sides:
        _sides[(name, k, t)] = Side(fhe, name, k, t)
    return _sides[(name, k, t)]


def _ptr(x):
    return C.c_void_p(x.data_ptr()) if x is not None else None


def _decrypt(fhe, ctx, sk_ntt, cts, noise=True, plain=None, unwritten=True):
    """the C ABI itself -> (plaintexts [count][n] uint64, noise bit lengths [count] or None); outputs start as garbage; unwritten: the
    input is compared with a copy taken before the call"""
    import torch
    count, size = int(cts.shape[0]), int(cts.shape[1])
    if plain is None:
        plain = torch.full((count, ctx.n), SENTINEL, dtype=torch.int64, device=ctx.device)
    bits = torch.full((count,), 0x55555555, dtype=torch.int32, device=ctx.device) if noise else None
    need = int(fhe._lib.load().fhe_decrypt_scratch_bytes(ctx.h, size, count))
    assert need == count * (size + 1) * ctx.k * ctx.n * 8
    scratch = torch.empty(need // 8, dtype=torch.int64, device=ctx.device)
    keep = cts.clone() if unwritten else None
    assert fhe._lib.call("fhe_decrypt_batch", ctx.h, _ptr(sk_ntt), _ptr(cts), size, count, _ptr(plain), _ptr(bits), _ptr(scratch), need, None) == 0
    torch.cuda.synchronize()
    assert keep is None or torch.equal(cts, keep), "the input was written"
    return plain, bits


def _host(t):
    return t.cpu().numpy().view(np.uint64) if t.dtype.itemsize == 8 else t.cpu().numpy()


def _cts(fhe, ctx, rows):
    """phases [count][k][n] (uint64 residues) -> size-2 ciphertexts (c_0 = phase, c_1 = 0) on the device"""
    rows = np.asarray(rows, dtype=np.uint64)
    ct = np.zeros((rows.shape[0], 2) + rows.shape[1:], dtype=np.uint64)
    ct[:, 0] = rows
    return fhe.to_device(ct, ctx.device)


def _want(cr, x):
    return np.array([dc.plain_of(v, cr.Q, cr.t) for v in x], dtype=np.uint64), cr.bits(x)


def _first_bad(got, want):
    bad = np.argwhere(got != want)
    return "%d coefficients differ, first (ciphertext, index) %s: got %d, want %d" % (len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]) if bad.size else ""


@pytest.mark.parametrize("name,k,t", dc.CASES, ids=["%s-k%d-t%d" % c for c in dc.CASES])
def test_rounding_at_its_edges(fhe, oracle_mod, name, k, t):
    s = _side(fhe, name, k, t)
    cr, ctx = s.cr, s.ctx
    print("\n%s t=%d: ctx.k = %d (k_dec_round<%d>), q of %d bits" % (name, cr.t, ctx.k, ctx.k, s.qbits))
    rng = random.Random("row/%s/%d/%d" % (name, k, t))
    xs = [cr.x, cr.x[::-1], [rng.randrange(cr.Q) for _ in range(cr.n)]]
    want = [_want(cr, x) for x in xs]
    assert np.array_equal(want[0][0], np.array(cr.want_plain, dtype=np.uint64)) and want[0][1] == max(b for _, b, _ in cr.model)
    want_plain, want_bits = np.stack([w[0] for w in want]), [w[1] for w in want]
    cts = _cts(fhe, ctx, [cr.residues(x) for x in xs])
    plain, bits = _decrypt(fhe, ctx, s.dec._sk_ntt, cts)
    msg = _first_bad(_host(plain), want_plain)
    assert not msg, msg + " (crafted families: %s)" % sorted(key for key, pos in cr.where.items() if _host(plain)[0, pos] != want_plain[0, pos])[:8]
    assert _host(bits).tolist() == want_bits
    plain2, _ = _decrypt(fhe, ctx, s.dec._sk_ntt, cts, noise=False)             # d_noise_bits = NULL: the same plaintexts
    assert np.array_equal(_host(plain2), want_plain)
    p, budgets = s.dec.decrypt_batch(cts, with_budget=True)
    assert np.array_equal(p, want_plain) and budgets == [max(0, s.qbits - b - 1) for b in want_bits]
    if (name, k, t) in dc.WIDTHS:                                                # the two independent host decryptions, one base per prime width
        hp, hb = s.dec.decrypt_host(cts[0], with_budget=True)
        assert np.array_equal(hp, want_plain[0]) and hb == dc.budget_of(want_bits[0], cr.Q)
        orc = oracle_mod.Oracle(cr.n, cr.q, cr.t)
        op, nb, mb = orc.decrypt_noise_bits(fhe.to_host(s.kg.secret_key()), fhe.to_host(cts[0]))
        assert np.array_equal(op, want_plain[0]) and (nb, mb) == (want_bits[0], s.qbits)


@pytest.mark.parametrize("name,k,t", dc.CASES, ids=["%s-k%d-t%d" % c for c in dc.CASES])
def test_every_noise_length_alone_in_a_quiet_ciphertext(fhe, name, k, t):
    s = _side(fhe, name, k, t)
    cr, ctx, n = s.cr, s.ctx, s.cr.n
    rows = np.zeros((len(cr.quiet), k, n), dtype=np.uint64)
    want_plain = np.zeros((len(cr.quiet), n), dtype=np.uint64)
    want_bits = []
    for e, (lab, v, pos) in enumerate(cr.quiet):
        x = cr.with_noise(v)
        assert dc.noise_of(x, cr.Q, cr.t) == abs(v)
        rows[e, :, pos] = [x % p for p in cr.q]
        want_plain[e, pos] = dc.plain_of(x, cr.Q, cr.t)
        want_bits.append(abs(v).bit_length())
    print("\n%s t=%d: ctx.k = %d, %d quiet ciphertexts, figures %s" % (name, cr.t, ctx.k, len(cr.quiet), sorted(set(want_bits))))
    cts = _cts(fhe, ctx, rows)
    plain, bits = _decrypt(fhe, ctx, s.dec._sk_ntt, cts)
    got = _host(bits).tolist()
    assert got == want_bits, [(cr.quiet[e][0], g, w) for e, (g, w) in enumerate(zip(got, want_bits)) if g != w][:8]
    msg = _first_bad(_host(plain), want_plain)
    assert not msg, msg
    p, budgets = s.dec.decrypt_batch(cts, with_budget=True)
    assert np.array_equal(p, want_plain) and budgets == [s.qbits - b - 1 for b in want_bits] and min(budgets) >= 0 and max(budgets) == s.qbits - 1


def test_noise_figure_is_a_per_ciphertext_maximum(fhe):
    s = _side(fhe, "Q4", 3, 65537)
    cr, ctx, n = s.cr, s.ctx, s.cr.n
    loud = {1: (1 << 64) - 1, 3: -(1 << 64)}                                     # noise 2^64 - 1: 64 bits; 2^64: 65 bits
    rng = random.Random("loud")
    for pos in (0, n - 1, 64 * rng.randrange(1, n // 64 - 1) + rng.randrange(1, 63)):
        xs = [[0] * n for _ in range(5)]
        for e, v in loud.items():
            xs[e][pos] = cr.with_noise(v)
            assert dc.noise_of(xs[e][pos], cr.Q, cr.t) == abs(v)
        plain, bits = _decrypt(fhe, ctx, s.dec._sk_ntt, _cts(fhe, ctx, [cr.residues(x) for x in xs]))
        assert _host(bits).tolist() == [0, 64, 0, 65, 0], pos
        assert np.array_equal(_host(plain), np.stack([_want(cr, x)[0] for x in xs]))


@pytest.mark.parametrize("name,k,t", [("W61", 2, (1 << 59) + 1), ("Q4", 4, 65537), ("Q3", 3, 12289)], ids=["W61-k2", "Q4-k4", "Q3-k3"])
def test_horner_at_its_edges(fhe, name, k, t):
    s = _side(fhe, name, k, t)
    cr, ctx, n, q = s.cr, s.ctx, s.cr.n, s.cr.q
    print("\n%s: ctx.k = %d" % (name, ctx.k))
    crt = [P * ip for P, ip in zip(cr.C.punct, cr.C.inv_punct)]
    rng = np.random.default_rng(dc.SEED + k)
    for size in (2, 3, 5, _header(fhe, "FHE_MAX_POLYS")):
        ct = np.zeros((3, size, k, n), dtype=np.uint64)
        for i, p in enumerate(q):
            ct[0, :, i] = p - 1                                                  # every operand of mul_barrett / addmod at q_i - 1
            ct[1, size - 1, i] = p - 1                                           # all 0 except the last polynomial
            ct[2, :, i] = rng.integers(0, p, size=(size, n), dtype=np.uint64)
        d_ct = fhe.to_device(ct, ctx.device)
        for label, key in (("-1", [p - 1 for p in q]), ("1", [1] * k), ("q/2+1", [p // 2 + 1 for p in q])):
            sk_ntt = fhe.to_device(np.array([[sv] * n for sv in key], dtype=np.uint64), ctx.device)
            plain, bits = _decrypt(fhe, ctx, sk_ntt, d_ct)
            for e in range(3):
                phase = []
                for i, p in enumerate(q):                                        # sum_j c_j s_i^j mod q_i per coefficient, Python integers
                    acc = ct[e, size - 1, i].astype(object)
                    for j in range(size - 2, -1, -1):
                        acc = (acc * key[i] + ct[e, j, i].astype(object)) % p
                    phase.append(acc)
                x = [sum(int(phase[i][c]) * crt[i] for i in range(k)) % cr.Q for c in range(n)]
                wp, wb = _want(cr, x)
                msg = _first_bad(_host(plain)[e:e + 1], wp[None])
                assert not msg, (size, label, e, msg)
                assert int(_host(bits)[e]) == wb, (size, label, e)


def test_both_grid_stride_loops_take_a_second_trip(fhe):
    import torch
    s = _side(fhe, "Q3", 2, 12289)
    cr, ctx, n = s.cr, s.ctx, s.cr.n
    rng = random.Random("block")
    xs = [cr.x, cr.x[::-1]] + [[rng.randrange(cr.Q) for _ in range(n)] for _ in range(62)]
    block = _cts(fhe, ctx, [cr.residues(x) for x in xs])
    plain, bits = _decrypt(fhe, ctx, s.dec._sk_ntt, block)                       # only this block meets the CPU reference
    want = [_want(cr, x) for x in xs]
    assert np.array_equal(_host(plain), np.stack([w[0] for w in want])) and _host(bits).tolist() == [w[1] for w in want]
    reps = 257
    count = 64 * reps
    assert count * n > 65535 * 256 and count * ctx.k > 32768
    big = block.repeat(reps, 1, 1, 1)                                            # [count][2][k][n]: 0.54 GB, + 0.81 GB of scratch, 0.13 GB of plaintexts
    assert big.shape == (count, 2, ctx.k, n)
    got_plain, got_bits = _decrypt(fhe, ctx, s.dec._sk_ntt, big, unwritten=False)    # no second copy of the input: the block's call above checked that
    del big
    assert got_plain.shape == (count, n) and torch.equal(got_plain.view(reps, 64, n), plain[None].expand(reps, 64, n))
    assert torch.equal(got_bits.view(reps, 64), bits[None].expand(reps, 64))


def test_refusals_leave_the_output_untouched(fhe):
    import torch
    L = fhe._lib.load()

    def refused(ctx, what, sk_ntt, cts, size, count, scratch, scratch_bytes):
        plain = torch.full((2, ctx.n), SENTINEL, dtype=torch.int64, device=ctx.device)
        bits = torch.full((2,), 0x55555555, dtype=torch.int32, device=ctx.device)
        with pytest.raises(fhe.FheError) as err:
            fhe._lib.call("fhe_decrypt_batch", ctx.h, _ptr(sk_ntt), _ptr(cts), size, count, _ptr(plain), _ptr(bits), _ptr(scratch), scratch_bytes, None)
        assert err.value.code == _header(fhe, "FHE_ERR_PARAM") == -1, what
        torch.cuda.synchronize()
        assert bool((plain == SENTINEL).all()) and bool((bits == 0x55555555).all()), what
        return str(err.value)

    q = dc.primes("W61", 1)
    wide = fhe.SEALContext(dc.N, q, 1 << 60)                                      # below the prime, so a context exists; decryption refuses
    need = int(L.fhe_decrypt_scratch_bytes(wide.h, 2, 2))
    scratch = torch.empty(need // 8, dtype=torch.int64, device=wide.device)
    key = torch.ones((1, dc.N), dtype=torch.int64, device=wide.device)
    assert "plain modulus too large" in refused(wide, "t = 2^60", key, wide.random_ct(2), 2, 2, scratch, need)
    s = _side(fhe, "Q3", 2, 12289)
    ctx, sk = s.ctx, s.dec._sk_ntt
    cts = ctx.random_ct(2)
    need = int(L.fhe_decrypt_scratch_bytes(ctx.h, 2, 2))
    scratch = torch.empty(need // 8, dtype=torch.int64, device=ctx.device)
    refused(ctx, "size 1", sk, cts, 1, 2, scratch, need)
    refused(ctx, "null scratch", sk, cts, 2, 2, None, need)
    refused(ctx, "scratch 8 bytes short", sk, cts, 2, 2, scratch, need - 8)
    refused(ctx, "null key", None, cts, 2, 2, scratch, need)
    plain = torch.full((2, ctx.n), SENTINEL, dtype=torch.int64, device=ctx.device)
    assert fhe._lib.call("fhe_decrypt_batch", ctx.h, _ptr(sk), _ptr(cts), 2, 0, _ptr(plain), None, _ptr(scratch), need, None) == 0      # count = 0: FHE_OK
    torch.cuda.synchronize()
    assert bool((plain == SENTINEL).all())
    got, _ = _decrypt(fhe, ctx, sk, cts)                                         # and the same arguments, complete, decrypt
    assert not bool((got == SENTINEL).any())
