"""GPU: the hosts of the key switch with a special prime on real keys (KeyGenerator.generate_special_evaluation_keys /
generate_special_galois_keys, Evaluator.relinearize_sp, apply_galois / rotate_rows / rotate_columns with SpecialGaloisKeys, the C++
facade's seal::hip::relinearize_sp / rotate_rows_sp / rotate_columns_sp): results decrypt to what they must, every key switch keeps the
budget circuits.special_key_switch_budget promises, and the budgets are printed beside those of the dbc 30 / dbc 60 key switches at the
same level."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import galois_oracle as go

pytestmark = pytest.mark.gpu

N = 1024
# name -> (primes of the parent context, plain modulus: a prime = 1 (mod 2n))
PARENTS = {"P4096": (go.Q3, 12289), "P8192": (go.Q4, 65537)}
TILE_W = 32
_cache = {}


def _steps_needed():
    return sorted({(j - 1) * TILE_W + (i - 1) for j in range(3) for i in range(3)} - {0} | {1, -1, 4, -4})


def _setup(fhe, name):
    if name not in _cache:
        q, t = PARENTS[name]
        parent = fhe.SEALContext(N, q, t)
        L = parent.k - 1
        level = parent.level(L)
        kg = fhe.KeyGenerator(parent, seed=23)
        sk = kg.secret_key()[:L].contiguous()
        kgl = fhe.KeyGenerator(level, seed=29, secret_key=sk)             # the public key and the bit-decomposition keys AT the level
        ev = fhe.Evaluator(level)
        elements = [fhe.galois_element(N, s) for s in _steps_needed()] + [2 * N - 1]
        _cache[name] = dict(parent=parent, level=level, kg=kg, kgl=kgl, ev=ev, L=L,
                            enc=fhe.DeviceEncryptor(level, kgl.public_key(), key=bytes(range(32)), reproducible=True),
                            dec=fhe.Decryptor(level, sk), be=fhe.BatchEncoder(level), elements=elements,
                            rk=kg.generate_special_evaluation_keys(1), gk=kg.generate_special_galois_keys(elements))
    return _cache[name]


def _exact_budgets(fhe, S, cts):
    """the invariant noise budget -log2(2 ||v||) of every ciphertext, exactly (the phase from the device, CRT and rounding in Python
    integers), beside the plaintexts: decrypt_batch's own figure is this rounded to a whole bit either way"""
    dec, t = S["dec"], S["level"].t
    out, plains = [], []
    for ct in cts:
        ph = dec._phase(ct)
        worst, plain = 0, np.zeros(N, dtype=np.uint64)
        for c in range(N):
            x = sum(int(ph[i, c]) * f for i, f in enumerate(dec._crt)) % dec.Q
            m = (t * x + dec.Q // 2) // dec.Q
            worst = max(worst, abs(t * x - m * dec.Q))
            plain[c] = m % t
        out.append(math.log2(dec.Q) - math.log2(worst) - 1)
        plains.append(plain)
    return out, np.stack(plains)


@pytest.mark.parametrize("name", list(PARENTS))
def test_key_shapes(fhe, name):
    S = _setup(fhe, name)
    parent, L = S["parent"], S["L"]
    assert tuple(S["rk"].shape) == (1, L, 2, parent.k, N) and S["rk"].numel() == fhe._lib.load().fhe_ksk_sp_words(parent.h)
    gk = S["gk"]
    assert isinstance(gk, fhe.SpecialGaloisKeys) and gk.ctx is parent and gk.elements() == sorted(set(S["elements"]))
    assert gk.has(3) and not gk.has(7) and tuple(gk.key(3).shape) == (L, 2, parent.k, N)
    with pytest.raises(ValueError, match="no Galois key"):
        gk.key(7)
    two = S["kg"].generate_special_evaluation_keys(2)
    assert tuple(two.shape) == (2, L, 2, parent.k, N)
    one = fhe.SEALContext(N, parent.q[:1], parent.t)
    for make in (lambda g: g.generate_special_evaluation_keys(), lambda g: g.generate_special_galois_keys([3])):
        with pytest.raises(ValueError, match="at least 2 primes"):
            make(fhe.KeyGenerator(one, seed=1))


@pytest.mark.parametrize("name", list(PARENTS))
def test_multiply_then_relinearize_sp(fhe, name):
    import torch
    S = _setup(fhe, name)
    parent, level, ev, be, t = S["parent"], S["level"], S["ev"], S["be"], S["level"].t
    rng = np.random.default_rng(1)
    a, b = (rng.integers(0, t, size=(2, N), dtype=np.uint64) for _ in range(2))
    S["enc"].seek(0)
    ca, cb = S["enc"].encrypt_plains(be.encode(a)), S["enc"].encrypt_plains(be.encode(b))
    prod = ev.multiply(ca, cb)
    want = (a.astype(object) * b.astype(object) % t).astype(np.uint64)
    before, plain = _exact_budgets(fhe, S, prod)
    assert np.array_equal(be.decode(plain), want)
    out = ev.relinearize_sp(prod, S["rk"], parent)
    assert tuple(out.shape) == (2, 2, level.k, N)
    after, plain = _exact_budgets(fhe, S, out)
    assert np.array_equal(be.decode(plain), want)
    line = []
    for bb, aa in zip(before, after):
        bound = fhe.circuits.special_key_switch_budget(parent, bb)
        assert aa >= bound - 1e-9, (name, bb, aa, bound)
        line.append("%.2f -> %.2f (bound %.2f)" % (bb, aa, bound))
    same = {}
    for dbc in (30, 60):                                               # SEAL 2.3's bit decomposition at the SAME level
        evk = S["kgl"].generate_evaluation_keys(dbc)
        same[dbc] = S["dec"].decrypt_batch(ev.relinearize(prod, evk, dbc), with_budget=True)[1]
    print("\n[relinearize_sp %s n=%d level of %d primes] exact budget %s; whole bits: special %r, dbc 30 %r, dbc 60 %r"
          % (name, N, level.k, "; ".join(line), S["dec"].decrypt_batch(out, with_budget=True)[1], same[30], same[60]))
    # a size-4 ciphertext goes down in two steps, top polynomial first: the C ABI's steps by hand give the same bytes
    keys2 = S["kg"].generate_special_evaluation_keys(2)
    four = level.random_ct(2, size=4)
    got = ev.relinearize_sp(four, keys2, parent)
    work = four.clone()
    L, kn = S["L"], level.k * N
    lib = fhe._lib.load()
    nbytes = lib.fhe_key_switch_sp_scratch_bytes(parent.h, 2)
    scr = torch.empty(nbytes // 8, dtype=torch.int64, device=level.device)
    import ctypes as C
    p = lambda x: C.c_void_p(x.data_ptr())
    for sp in (3, 2):
        fhe._lib.call("fhe_relinearize_sp_poly", parent.h, p(work), 4 * kn, sp, p(work), 4 * kn, 2, p(keys2[sp - 2]), p(scr), nbytes, None)
    assert torch.equal(got, work[:, :2])
    assert ev.relinearize_sp(ca, S["rk"], parent) is ca                 # size 2: nothing to do
    with pytest.raises(ValueError, match="key set"):
        ev.relinearize_sp(four, S["rk"], parent)


@pytest.mark.parametrize("name", list(PARENTS))
def test_rotations(fhe, name):
    import torch
    S = _setup(fhe, name)
    parent, level, ev, be, gk, t = S["parent"], S["level"], S["ev"], S["be"], S["gk"], S["level"].t
    rng = np.random.default_rng(2)
    slots = rng.integers(0, t, size=(2, N), dtype=np.uint64)
    S["enc"].seek(10)
    ct = S["enc"].encrypt_plains(be.encode(slots))
    fresh, plain = _exact_budgets(fhe, S, ct)
    assert np.array_equal(be.decode(plain), slots)
    lines = []
    for steps in (1, -1, 5, -5):
        plan = ev.rotation_plan(steps, gk)
        assert len(plan) == (1 if abs(steps) == 1 else 2)
        out = ev.rotate_rows(ct, steps, gk)
        after, plain = _exact_budgets(fhe, S, out)
        assert np.array_equal(be.decode(plain), go.permute_slots(slots, steps, False)), steps
        for f, a in zip(fresh, after):
            bound = f
            for _ in plan:
                bound = fhe.circuits.special_key_switch_budget(parent, bound)
            assert a >= bound - 1e-9, (name, steps, f, a, bound)
        lines.append("rows %+d: %.2f -> %.2f (bound %.2f)" % (steps, fresh[0], after[0], bound))
    out = ev.rotate_columns(ct, gk)
    after, plain = _exact_budgets(fhe, S, out)
    assert np.array_equal(be.decode(plain), go.permute_slots(slots, 0, True))
    assert all(a >= fhe.circuits.special_key_switch_budget(parent, f) - 1e-9 for f, a in zip(fresh, after))
    lines.append("columns: %.2f -> %.2f" % (fresh[0], after[0]))
    buf = ct.clone()
    assert ev.rotate_rows(buf, 5, gk, out=buf) is buf and torch.equal(buf, ev.rotate_rows(ct, 5, gk))
    same = {}
    for dbc in (30, 60):
        keys = S["kgl"].generate_galois_keys(dbc, elements=[3])
        same[dbc] = S["dec"].decrypt_batch(ev.rotate_rows(ct, 1, keys), with_budget=True)[1]
    whole = S["dec"].decrypt_batch(ev.rotate_rows(ct, 1, gk), with_budget=True)[1]
    print("\n[rotations, special prime, %s n=%d level of %d primes] exact budget %s; one rotation in whole bits from %r: special %r, dbc 30 %r, dbc 60 %r"
          % (name, N, level.k, "; ".join(lines), S["dec"].decrypt_batch(ct, with_budget=True)[1], whole, same[30], same[60]))


@pytest.mark.parametrize("name", list(PARENTS))
def test_packed_filter_with_special_keys(fhe, name):
    S = _setup(fhe, name)
    level, ev, be = S["level"], S["ev"], S["be"]
    th = N // 2 // TILE_W
    w = np.outer([1, 2, 1], [1, 2, 1])
    rng = np.random.default_rng(3)
    tiles = rng.integers(0, 256, size=(2, th, TILE_W))
    S["enc"].seek(20)
    ct = S["enc"].encrypt_plains(be.encode(tiles.reshape(1, N).astype(np.uint64)))
    out = fhe.circuits.packed_filter2d(ev, S["gk"], ct, TILE_W, w, 3, 3)
    plain, budget = S["dec"].decrypt_batch(out, with_budget=True)
    keys = S["kgl"].generate_galois_keys(30, elements=[g for g in S["elements"] if g != 2 * N - 1])
    ref = fhe.circuits.packed_filter2d(ev, keys, ct, TILE_W, w, 3, 3)
    plain_ref, budget_ref = S["dec"].decrypt_batch(ref, with_budget=True)
    print("\n[packed_filter2d gauss3 %s level of %d primes] budget left: special keys %r bits, dbc 30 keys at the same level %r bits" % (name, level.k, budget, budget_ref))
    assert min(budget) > 0 and min(budget_ref) > 0
    assert np.array_equal(be.decode(plain), be.decode(plain_ref))
    mask = fhe.circuits.packed_filter_valid_mask(N, TILE_W, 3, 3).reshape(2, th, TILE_W)
    want = np.zeros((2, th, TILE_W), dtype=np.int64)
    for y in range(1, th - 1):
        for x in range(1, TILE_W - 1):
            want[:, y, x] = (tiles[:, y - 1:y + 2, x - 1:x + 2] * w).sum(axis=(1, 2))
    assert int(want.max()) < level.t
    assert np.array_equal(be.decode(plain)[0].reshape(2, th, TILE_W)[mask], want[mask].astype(np.uint64))


def test_keys_of_another_parent_are_refused(fhe):
    S = _setup(fhe, "P8192")
    ev, level = S["ev"], S["level"]
    ct = level.random_ct(1)
    other = fhe.SEALContext(N, go.Q4[:2] + go.Q4[3:], S["parent"].t)   # another base: its first k - 1 primes are not this level's
    okeys = fhe.KeyGenerator(other, seed=3).generate_special_galois_keys([3])
    with pytest.raises(ValueError, match="another parent"):
        ev.apply_galois(ct, 3, okeys)
    with pytest.raises(ValueError, match="another parent"):
        ev.rotate_rows(ct, 1, okeys)
    with pytest.raises(ValueError, match="another parent"):
        fhe.Evaluator(S["parent"]).apply_galois(S["parent"].random_ct(1), 3, S["gk"])      # ciphertexts of the parent itself, not of its level
    with pytest.raises(ValueError, match="another parent"):
        ev.relinearize_sp(level.random_ct(1, size=3), S["rk"], other)
    with pytest.raises(ValueError, match="special-prime key"):
        ev.relinearize_sp(level.random_ct(1, size=3), S["rk"][:, :, :, :-1].contiguous(), S["parent"])
    with pytest.raises(ValueError, match="size 2"):
        ev.apply_galois(level.random_ct(1, size=3), 3, S["gk"])
    with pytest.raises(ValueError, match="no Galois key"):
        ev.apply_galois(ct, 7, S["gk"])


@pytest.mark.parametrize("name", list(PARENTS))
def test_cpp_host_agrees_with_the_python_host(fhe, tmp_path, name):
    """seal/keyswitch_sp_check (seal::hip::relinearize_sp, rotate_rows_sp, rotate_columns_sp) on a stream of size-3 ciphertexts: the bytes
    of the Python host"""
    exe = os.path.join(os.path.dirname(fhe.LIB_PATH), "seal", "keyswitch_sp_check")
    assert os.path.exists(exe), "build() makes seal/keyswitch_sp_check"
    S = _setup(fhe, name)
    parent, level, ev, gk = S["parent"], S["level"], S["ev"], S["gk"]
    ct = level.random_ct(3, size=3, seed=77)
    want = fhe.to_host(ev.rotate_columns(ev.rotate_rows(ev.relinearize_sp(ct, S["rk"], parent), -5, gk), gk))
    fin, fout, frk, fgk, fwant = (str(tmp_path / x) for x in ("in.ct", "out.ct", "relin.keys", "galois.keys", "want.ct"))
    with open(fin, "wb") as f:
        for c in fhe.to_host(ct):
            fhe.server.write_ciphertext(f, c)
    with open(frk, "wb") as f:
        f.write(fhe.to_host(S["rk"]).tobytes())
    with open(fgk, "wb") as f:
        for g in gk.elements():
            f.write(struct.pack("<2I", g, 0))
            f.write(fhe.to_host(gk.key(g)).tobytes())
    with open(fwant, "wb") as f:
        for c in want:
            fhe.server.write_ciphertext(f, c)
    r = subprocess.run([exe, fin, fout, "3", "3", frk, fgk, "-5", "1", str(N), str(parent.t)] + [str(q) for q in parent.q], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(fout, "rb").read() == open(fwant, "rb").read()
    digest = sum(int(w) * (2 * i + 1) for i, w in enumerate(want.reshape(-1))) % (1 << 64)
    assert "digest=%016x" % digest in r.stdout, r.stdout
