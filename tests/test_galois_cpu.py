"""CPU: the specification of the Galois rotations holds on the unchanged oracle (tests/galois_oracle.py), and the host-only entry
points of the library -- fhe_batch_encode / fhe_batch_decode, fhe_galois_element -- agree with its independent restatements."""
import ctypes as C

import numpy as np
import pytest

import galois_oracle as go


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("n", [64, 1024])
def test_specification_on_the_oracle(oracle_mod, n):
    """apply_galois as Oracle.relinearize of [sigma(c0), 0, sigma(c1)] with a key for sigma_g(s) decrypts to exactly the expected slot
    permutation: g = 3^s rotates both rows left by s, g = 2n - 1 swaps them"""
    t = go.T_BATCH
    orc = oracle_mod.Oracle(n, go.Q3, t)
    sk, pk = orc.keygen(seed=5)
    rng = np.random.default_rng(n)
    slots = rng.integers(0, t, size=n, dtype=np.uint64)
    plain = go.encode_slots(slots, n, t)
    assert np.array_equal(go.decode_slots(plain, n, t), slots)
    ct = orc.encrypt(pk, plain, seed=3)
    fresh_plain, fresh = orc.decrypt(sk, ct)
    assert np.array_equal(fresh_plain, plain)
    for dbc in (30, 60):
        for g, left, swap in go.elements(n):
            key = go.galois_key(orc, sk, g, dbc, seed=g + dbc)
            out = go.apply_galois(orc, ct, g, key, dbc)
            dec, budget = orc.decrypt(sk, out)
            print("[galois oracle n=%d dbc=%d g=%d] noise budget %d -> %d bits" % (n, dbc, g, fresh, budget))
            assert budget > 0
            assert np.array_equal(go.decode_slots(dec, n, t), go.permute_slots(slots, left, swap)), (n, dbc, g)


def test_sigma_is_a_ring_automorphism():
    """sigma_g(a b) = sigma_g(a) sigma_g(b) in Z_q[x] / (x^n + 1) (schoolbook product), and sigma_g sigma_g^-1 = id; zero stays zero"""
    n, q = 16, [97]
    rng = np.random.default_rng(2)
    a, b = (rng.integers(0, q[0], size=(1, n), dtype=np.uint64) for _ in range(2))
    a[0, 3] = 0

    def mul(x, y):
        out = [0] * n
        for i in range(n):
            for j in range(n):
                s = int(x[0, i]) * int(y[0, j])
                out[(i + j) % n] += s if i + j < n else -s
        return np.array([[v % q[0] for v in out]], dtype=np.uint64)
    for g in (3, 5, 2 * n - 1, pow(3, -1, 2 * n)):
        assert np.array_equal(go.sigma(mul(a, b), g, q), mul(go.sigma(a, g, q), go.sigma(b, g, q)))
        assert np.array_equal(go.sigma(go.sigma(a, g, q), pow(g, -1, 2 * n), q), a)
        assert (go.sigma(a, g, q) < q[0]).all()


@pytest.mark.parametrize("n,t", [(1024, 65537), (1024, 12289), (4096, 65537)])
def test_batch_encoder_matches_the_python_encoder(fhe, n, t):
    lib = fhe._lib.load()
    rng = np.random.default_rng(n + t)
    slots = np.stack([rng.integers(0, t, size=n, dtype=np.uint64), np.full(n, t - 1, dtype=np.uint64), np.zeros(n, dtype=np.uint64)])
    slots[2, 1], slots[2, n // 2] = 7, 9                               # one slot per row: pins the slot order
    plain = np.zeros_like(slots)
    assert lib.fhe_batch_encode(n, t, _vp(slots), len(slots), _vp(plain)) == 0
    for i in range(len(slots)):
        assert np.array_equal(plain[i], go.encode_slots(slots[i], n, t)), (n, t, i)
    back = np.zeros_like(slots)
    assert lib.fhe_batch_decode(n, t, _vp(plain), len(slots), _vp(back)) == 0
    assert np.array_equal(back, slots)
    assert np.array_equal(back[0], go.decode_slots(plain[0], n, t))
    other = rng.integers(0, t, size=(1, n), dtype=np.uint64)           # decode of a plaintext that no encode made
    assert lib.fhe_batch_decode(n, t, _vp(other), 1, _vp(back)) == 0
    assert np.array_equal(back[0], go.decode_slots(other[0], n, t))
    # slot-wise product: the ring product of two plaintexts holds the products of their slots
    if n == 1024:
        a, b = [int(x) for x in plain[0]], [int(x) for x in other[0]]
        prod = [0] * n
        for i in np.flatnonzero(plain[0]):
            for j in range(n):
                s = a[i] * b[j]
                prod[(i + j) % n] += s if i + j < n else -s
        prod = np.array([[v % t for v in prod]], dtype=np.uint64)
        assert lib.fhe_batch_decode(n, t, _vp(prod), 1, _vp(back)) == 0
        assert np.array_equal(back[0], slots[0] * go.decode_slots(other[0], n, t) % np.uint64(t))


def test_batch_encoder_refusals(fhe):
    lib = fhe._lib.load()
    n = 1024
    a, b = np.zeros((1, n), dtype=np.uint64), np.zeros((1, n), dtype=np.uint64)
    for t in (1 << 14, 65539, 65536 + 2049, 3):                         # the presets' 2^14; a prime that is not 1 mod 2n; a composite that is; too small
        assert t != 65536 + 2049 or (t % (2 * n) == 1 and not go.is_prime(t))
        assert t != 65539 or (go.is_prime(t) and t % (2 * n) != 1)
        assert lib.fhe_batch_encode(n, t, _vp(a), 1, _vp(b)) == -1, t
        assert lib.fhe_batch_decode(n, t, _vp(a), 1, _vp(b)) == -1, t
        assert b"batching needs a prime" in lib.fhe_last_error()
    a[0, 5] = 65537
    assert lib.fhe_batch_encode(n, 65537, _vp(a), 1, _vp(b)) == -1 and b">= t" in lib.fhe_last_error()
    assert lib.fhe_batch_decode(n, 65537, _vp(a), 1, _vp(b)) == -1
    a[0, 5] = 65536
    assert lib.fhe_batch_encode(n, 65537, _vp(a), 1, _vp(b)) == 0
    assert lib.fhe_batch_encode(1000, 65537, _vp(a), 1, _vp(b)) == -1   # not a power of two
    assert lib.fhe_batch_encode(n, 65537, None, 1, _vp(b)) == -1


def test_galois_element(fhe):
    lib = fhe._lib.load()
    for n in (64, 1024, 8192):
        g = C.c_uint32()
        for steps, want in ((1, 3), (-1, pow(3, -1, 2 * n)), (n // 4, pow(3, n // 4, 2 * n)), (0, 1), (5, pow(3, 5, 2 * n)), (-5, pow(3, -5, 2 * n)),
                            (n // 2 + 1, 3), (-(n // 8), pow(3, -(n // 8), 2 * n))):
            assert lib.fhe_galois_element(n, steps, 0, C.byref(g)) == 0 and g.value == want, (n, steps)
            assert fhe.galois_element(n, steps) == want
        assert lib.fhe_galois_element(n, 0, 1, C.byref(g)) == 0 and g.value == 2 * n - 1
        assert lib.fhe_galois_element(n, 2, 1, C.byref(g)) == 0 and g.value == 9 * (2 * n - 1) % (2 * n)
    assert lib.fhe_galois_element(1000, 1, 0, C.byref(g)) == -1
    assert lib.fhe_galois_element(1024, 1, 0, None) == -1


def test_apply_galois_refuses_null_arguments(fhe):
    """the checks that need no device: a null context is FHE_ERR_PARAM, and its scratch size is 0"""
    lib = fhe._lib.load()
    buf = np.zeros(8, dtype=np.uint64)
    assert lib.fhe_apply_galois(None, _vp(buf), 8, _vp(buf), 8, 1, 3, _vp(buf), 30, _vp(buf), 64, None) == -1
    assert b"null argument" in lib.fhe_last_error()
    assert lib.fhe_apply_galois_scratch_bytes(None, 30, 1) == 0
