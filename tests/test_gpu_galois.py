"""GPU: Galois rotations of encrypted slots (include/fhe_hip.h fhe_apply_galois; csrc/galois.hip) against the specification on the
unchanged CPU oracle (tests/galois_oracle.py): bit-exact on random residues and on the negation edges, fused path == staged path, in
place == out of place, strided == compact; rotations of real encryptions decrypt to the rotated slots; the packed filter; refusals."""
import ctypes as C

import numpy as np
import pytest

import galois_oracle as go

pytestmark = pytest.mark.gpu


def _is_prime(m):
    if m % 2 == 0:
        return False
    d, s = m - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        x = pow(a, d, m)
        if x in (1, m - 1):
            continue
        for _ in range(s - 1):
            x = x * x % m
            if x == m - 1:
                break
        else:
            return False
    return True


def _primes_58(n, count):
    """the largest `count` 58-bit primes = 1 (mod 2n): the pseudo-Mersenne class 2 of csrc/ntt_core.h"""
    out, m = [], (1 << 58) + 1
    while len(out) < count:
        m -= 2 * n
        if _is_prime(m):
            out.append(m)
    return out


# name -> (n, q, switches).  Q3 at its own n = 4096 runs the general path with the exact-FP64 transforms, "shoup" the general path with
# the Shoup transforms; Q4 is pseudo-Mersenne class 1, Q58 class 2.
BASES = {
    "Q3": (1024, go.Q3, {}),
    "Q4": (1024, go.Q4, {}),
    "Q58": (1024, None, {}),
    "shoup": (1024, go.Q4, {"FHE_NTT_NOPM": "1"}),
    "P4096": (4096, go.Q3, {}),
    "P8192": (8192, go.Q4, {}),
}
_cache = {}


def _setup(fhe, om, name, dbc):
    """(ctx, staged ctx, oracle, Evaluator, staged Evaluator, GaloisKeys, {g: the key in the oracle's form}), made once per (base, dbc)"""
    if (name, dbc) not in _cache:
        n, q, sw = BASES[name]
        q = _primes_58(n, 2) if q is None else q
        if name not in _cache:
            ctx = fhe.SEALContext(n, q, go.T_BATCH, switches=sw or None)
            staged = fhe.SEALContext(n, q, go.T_BATCH, switches=dict(sw, FHE_GALOIS_STAGED="1"))
            _cache[name] = (ctx, staged, om.Oracle(n, q, go.T_BATCH), fhe.KeyGenerator(ctx, seed=7))
        ctx, staged, orc, kg = _cache[name]
        ev = fhe.Evaluator(ctx)
        keys = kg.generate_galois_keys(dbc, elements=[g for g, _, _ in go.elements(n)])
        korc = {g: go.key_to_oracle(orc, fhe.to_host(ev.ntt_inverse(keys.key(g)))) for g in keys.elements()}
        _cache[(name, dbc)] = (ctx, staged, orc, ev, fhe.Evaluator(staged), keys, korc)
    return _cache[(name, dbc)]


def _gather_ev(fhe, name):
    """an Evaluator on a context whose fused digit kernel gathers through LDS instead of from global memory (FHE_GALOIS_GATHER_LDS=1)"""
    if ("gather", name) not in _cache:
        ctx = _cache[name][0]
        _cache[("gather", name)] = fhe.Evaluator(fhe.SEALContext(ctx.n, ctx.q, ctx.t, switches=dict(BASES[name][2], FHE_GALOIS_GATHER_LDS="1")))
    return _cache[("gather", name)]


def _unreduced(fhe, ctx, t):
    import torch
    cnt = torch.zeros(1, dtype=torch.int64, device=ctx.device)
    fhe._lib.call("fhe_count_unreduced", ctx.h, C.c_void_p(t.data_ptr()), t.numel() // ctx.n // ctx.k, C.c_void_p(cnt.data_ptr()), None)
    return int(cnt.cpu()[0])


@pytest.mark.parametrize("dbc", [30, 60])
@pytest.mark.parametrize("name", list(BASES))
def test_apply_galois_matches_the_specification(fhe, oracle_mod, name, dbc):
    import torch
    ctx, staged, orc, ev, ev_staged, keys, korc = _setup(fhe, oracle_mod, name, dbc)
    count = 3 if ctx.n == 1024 else 2
    kn = ctx.k * ctx.n
    ct = ctx.random_ct(count, seed=fhe.SEED + dbc)
    host = fhe.to_host(ct)
    L = fhe._lib.load()
    print("\n[galois %s n=%d k=%d dbc=%d] arith path %d" % (name, ctx.n, ctx.k, dbc, L.fhe_arith_path(ctx.h)))
    for g, _, _ in go.elements(ctx.n):
        want = np.stack([go.apply_galois(orc, host[c], g, korc[g], dbc) for c in range(count)])
        out = ev.apply_galois(ct, g, keys)
        assert np.array_equal(fhe.to_host(out), want), (name, dbc, g)
        assert torch.equal(ct, fhe.to_device(host, ctx.device)), "the input was written"
        assert torch.equal(ev_staged.apply_galois(ct, g, keys), out), "staged path differs"
        assert torch.equal(_gather_ev(fhe, name).apply_galois(ct, g, keys), out), "LDS-gather variant differs"
        buf = ct.clone()
        assert ev.apply_galois(buf, g, keys, out=buf) is buf and torch.equal(buf, out), "in place differs"
        buf = ct.clone()
        assert torch.equal(ev_staged.apply_galois(buf, g, keys, out=buf), out), "staged in place differs"
        # a strided batch (gaps between the ciphertexts on both sides) through the C ABI
        si, so = 2 * kn + 3 * ctx.n, 2 * kn + 5 * ctx.n
        src = torch.full((count, si), -1, dtype=torch.int64, device=ctx.device)
        dst = torch.full((count, so), -1, dtype=torch.int64, device=ctx.device)
        src[:, :2 * kn] = ct.reshape(count, 2 * kn)
        nbytes = L.fhe_apply_galois_scratch_bytes(ctx.h, dbc, count)
        scr = torch.empty(nbytes // 8, dtype=torch.int64, device=ctx.device)
        p = lambda t: C.c_void_p(t.data_ptr())
        fhe._lib.call("fhe_apply_galois", ctx.h, p(src), si, p(dst), so, count, g, p(keys.key(g)), dbc, p(scr), nbytes, None)
        assert torch.equal(dst[:, :2 * kn].reshape(out.shape), out) and bool((dst[:, 2 * kn:] == -1).all()), "strided batch differs"


@pytest.mark.parametrize("dbc", [30, 60])
@pytest.mark.parametrize("name", ["Q3", "Q4", "Q58", "shoup"])
def test_negation_edges(fhe, oracle_mod, name, dbc):
    """every coefficient q_i - 1 (each negation gives 1), all zero (the negation of 0 is 0, not q_i), and zero except one coefficient per
    polynomial: the oracle's bits, and no residue at or above its modulus"""
    ctx, staged, orc, ev, ev_staged, keys, korc = _setup(fhe, oracle_mod, name, dbc)
    n, k = ctx.n, ctx.k
    qm1 = np.array(ctx.q, dtype=np.uint64)[None, :, None] - np.uint64(1)
    top = np.broadcast_to(qm1, (2, k, n)).copy()
    one = np.zeros((2, k, n), dtype=np.uint64)
    one[0, :, 1], one[1, :, n - 1] = qm1[0, :, 0], 5
    host = np.stack([top, np.zeros((2, k, n), dtype=np.uint64), one])
    ct = fhe.to_device(host, ctx.device)
    for g, _, _ in go.elements(n):
        want = np.stack([go.apply_galois(orc, host[c], g, korc[g], dbc) for c in range(3)])
        for e in (ev, ev_staged):
            out = e.apply_galois(ct, g, keys)
            assert np.array_equal(fhe.to_host(out), want), (name, dbc, g)
            assert _unreduced(fhe, ctx, out) == 0
        assert not fhe.to_host(out)[1].any()


def _client(fhe, name="Q3", dbc=30):
    key = ("client", name, dbc)
    if key not in _cache:
        n, q, _ = BASES[name]
        ctx = fhe.SEALContext(n, q, go.T_BATCH)
        kg = fhe.KeyGenerator(ctx, seed=11)
        _cache[key] = (ctx, kg, kg.generate_galois_keys(dbc), fhe.DeviceEncryptor(ctx, kg.public_key(), key=bytes(range(32)), reproducible=True),
                       fhe.Decryptor(ctx, kg.secret_key()), fhe.BatchEncoder(ctx), fhe.Evaluator(ctx))
    return _cache[key]


@pytest.mark.parametrize("dbc", [30, 60])
def test_rotations_decrypt_to_the_rotated_slots(fhe, dbc):
    import torch
    ctx, kg, keys, enc, dec, be, ev = _client(fhe, dbc=dbc)
    n = ctx.n
    assert sorted(keys.elements()) == sorted(set([pow(3, s * (1 << i), 2 * n) for i in range(9) for s in (1, -1)] + [2 * n - 1]))
    rng = np.random.default_rng(dbc)
    slots = rng.integers(0, ctx.t, size=(2, n), dtype=np.uint64)
    ct = enc.encrypt_plains(be.encode(slots))
    plain, fresh = dec.decrypt_batch(ct, with_budget=True)
    assert np.array_equal(be.decode(plain), slots)
    for steps in (1, -1, 5, n // 4, 0, n // 2 + 1, -(n // 4)):
        out = ev.rotate_rows(ct, steps, keys)
        plain, budget = dec.decrypt_batch(out, with_budget=True)
        print("[rotate_rows n=%d dbc=%d steps=%d] hops %d, noise budget %r -> %r bits" % (n, dbc, steps, len(ev.rotation_plan(steps, keys)), fresh, budget))
        assert min(budget) > 0
        assert np.array_equal(be.decode(plain), go.permute_slots(slots, steps, False)), steps
    out = ev.rotate_columns(ct, keys)
    plain, budget = dec.decrypt_batch(out, with_budget=True)
    print("[rotate_columns n=%d dbc=%d] noise budget %r -> %r bits" % (n, dbc, fresh, budget))
    assert min(budget) > 0 and np.array_equal(be.decode(plain), go.permute_slots(slots, 0, True))
    # a multi-hop rotation is the stated sequence of apply_galois calls, bit for bit
    assert ev.rotation_plan(5, keys) == [3, pow(3, 4, 2 * n)] and ev.rotation_plan(-5, keys) == [pow(3, -1, 2 * n), pow(3, -4, 2 * n)]
    assert ev.rotation_plan(n // 4, keys) == [pow(3, n // 4, 2 * n)] and ev.rotation_plan(0, keys) == [] and ev.rotation_plan(n // 2, keys) == []
    want = ev.apply_galois(ev.apply_galois(ct, 3, keys), pow(3, 4, 2 * n), keys)
    assert torch.equal(ev.rotate_rows(ct, 5, keys), want)
    buf = ct.clone()
    assert ev.rotate_rows(buf, 5, keys, out=buf) is buf and torch.equal(buf, want)
    assert torch.equal(ev.rotate_rows(ct, 0, keys), ct) and ev.rotate_rows(ct, 0, keys) is not ct
    # with the element itself in the key set the same rotation is one apply_galois
    direct = kg.generate_galois_keys(dbc, elements=[pow(3, 5, 2 * n)])
    assert ev.rotation_plan(5, direct) == [pow(3, 5, 2 * n)]
    plain = dec.decrypt_batch(ev.rotate_rows(ct, 5, direct))
    assert np.array_equal(be.decode(plain), go.permute_slots(slots, 5, False))


@pytest.mark.parametrize("kernel", ["box3", "gauss3"])
def test_packed_filter(fhe, kernel):
    """two 32 x 16 tiles in one ciphertext at n = 1024: packed_filter2d decrypts, on the valid mask, to the integer filter exactly, and
    is the op-by-op Evaluator sequence of its specification"""
    import torch
    ctx, kg, keys, enc, dec, be, ev = _client(fhe)
    n, tw, th = ctx.n, 32, 16
    w = np.ones((3, 3), dtype=np.int64) if kernel == "box3" else np.outer([1, 2, 1], [1, 2, 1])
    rng = np.random.default_rng(3)
    tiles = rng.integers(0, 256, size=(2, th, tw))
    ct = enc.encrypt_plains(be.encode(tiles.reshape(1, n).astype(np.uint64)))
    out = fhe.circuits.packed_filter2d(ev, keys, ct, tw, w, 3, 3)
    plain, budget = dec.decrypt_batch(out, with_budget=True)
    print("\n[packed_filter2d %s] noise budget left %r bits" % (kernel, budget))
    assert min(budget) > 0
    got = be.decode(plain)[0].reshape(2, th, tw)
    mask = fhe.circuits.packed_filter_valid_mask(n, tw, 3, 3).reshape(2, th, tw)
    assert mask.sum() == 2 * (th - 2) * (tw - 2) and not mask[:, 0].any() and not mask[:, :, -1].any()
    want = np.zeros((2, th, tw), dtype=np.int64)
    for y in range(1, th - 1):
        for x in range(1, tw - 1):
            want[:, y, x] = (tiles[:, y - 1:y + 2, x - 1:x + 2] * w).sum(axis=(1, 2))
    assert int(want.max()) < ctx.t
    assert np.array_equal(got[mask], want[mask].astype(np.uint64))
    acc = None
    for p, wp in enumerate(w.reshape(-1)):
        j, i = divmod(p, 3)
        term = ev.multiply_plain(ev.rotate_rows(ct, (j - 1) * tw + (i - 1), keys), np.array([int(wp)], dtype=np.uint64))
        acc = term if acc is None else ev.add(acc, term)
    assert torch.equal(out, acc)


def test_refusals(fhe):
    """every bad operand is an error before the first launch: the output keeps its sentinel"""
    import torch
    ctx, kg, keys, enc, dec, be, ev = _client(fhe)
    n, kn = ctx.n, ctx.k * ctx.n
    L = fhe._lib.load()
    ct = ctx.random_ct(2)
    out = torch.full_like(ct, -1)
    key = keys.key(3)
    nbytes = L.fhe_apply_galois_scratch_bytes(ctx.h, 30, 2)
    scr = torch.empty(nbytes // 8, dtype=torch.int64, device=ctx.device)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(src=ct, stride=2 * kn, dst=out, ostride=2 * kn, count=2, g=3, k=key, dbc=30, s=scr, sb=nbytes):
        return L.fhe_apply_galois(ctx.h, p(src) if src is not None else None, stride, dst if isinstance(dst, C.c_void_p) else p(dst), ostride, count, g,
                                  p(k) if k is not None else None, dbc, p(s) if s is not None else None, sb, None)
    assert call(g=4) == -1 and b"Galois element" in L.fhe_last_error()
    assert call(g=2 * n) == -1 and call(g=2 * n + 1) == -1 and call(g=1) == -1 and call(g=0) == -1
    assert call(sb=nbytes - 8) == -1 and b"scratch" in L.fhe_last_error()
    assert call(s=None) == -1
    assert call(dbc=0) == -1 and call(dbc=61) == -1
    assert call(stride=2 * kn - 1) == -1 and call(ostride=kn) == -1
    assert call(src=None) == -1 and call(k=None) == -1
    inside = C.c_void_p(ct.data_ptr() + 8 * kn)                        # the output inside the input range
    assert call(dst=inside, count=1) == -1 and b"overlaps" in L.fhe_last_error()
    assert call(dst=ct, ostride=4 * kn, count=1) == -1                 # same pointer, another stride
    assert call(s=ct, sb=nbytes) == -1 and b"scratch overlaps" in L.fhe_last_error()
    assert call(count=0) == 0
    torch.cuda.synchronize()
    assert bool((out == -1).all()), "a refused call wrote its output"
    with pytest.raises(ValueError, match="size 2"):
        ev.apply_galois(ctx.random_ct(1, size=3), 3, keys)
    with pytest.raises(ValueError, match="size 2"):
        ev.rotate_rows(ctx.random_ct(1, size=3), 0, keys)
    with pytest.raises(ValueError, match="`out`"):
        ev.rotate_rows(ct, 0, keys, out=torch.empty(1, 2, ctx.k, n, dtype=torch.int64, device=ctx.device))
    with pytest.raises(ValueError, match="Galois element"):
        ev.apply_galois(ct, 6, keys)
    with pytest.raises(ValueError, match="no Galois key"):
        ev.apply_galois(ct, 7, keys)
    other = fhe.SEALContext(2048, go.Q3, go.T_BATCH)
    with pytest.raises(ValueError, match="another context"):
        ev.apply_galois(ct, 3, fhe.KeyGenerator(other, seed=1).generate_galois_keys(30, elements=[3]))
    for wrong in (60, 15):                                             # keys made at dbc 30 presented as another dbc: fewer / more digits
        with pytest.raises(ValueError, match="evaluation keys|key set"):
            ev.apply_galois(ct, 3, fhe.GaloisKeys(ctx, wrong, {3: key}))
    with pytest.raises(ValueError, match="`out`"):
        ev.apply_galois(ct, 3, keys, out=torch.empty(1, 2, ctx.k, n, dtype=torch.int64, device=ctx.device))
    with pytest.raises(fhe.FheError, match="batching needs a prime"):
        fhe.BatchEncoder(fhe.SEALContext(n, go.Q3, 1 << 14))


def test_cpp_host_agrees_with_the_python_host(fhe, tmp_path):
    """seal/galois_check (seal::hip::rotate_rows / rotate_columns over the facade) on a stream of packed ciphertexts: the bytes of the Python host"""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(fhe.LIB_PATH), "seal", "galois_check")
    assert os.path.exists(exe), "build() makes seal/galois_check"
    ctx, kg, keys, enc, dec, be, ev = _client(fhe)
    rng = np.random.default_rng(8)
    ct = enc.encrypt_plains(be.encode(rng.integers(0, ctx.t, size=(2, ctx.n), dtype=np.uint64)))
    fin, fout, fkeys = (str(tmp_path / x) for x in ("in.ct", "out.ct", "galois.keys"))
    with open(fin, "wb") as f:
        for c in fhe.to_host(ct):
            fhe.server.write_ciphertext(f, c)
    with open(fkeys, "wb") as f:
        keys.save(f)
    want = fhe.to_host(ev.rotate_columns(ev.rotate_rows(ct, -37, keys), keys))
    r = subprocess.run([exe, fin, fout, "2", fkeys, "-37", "1", str(ctx.n), str(ctx.t)] + [str(q) for q in ctx.q], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    fwant = str(tmp_path / "want.ct")
    with open(fwant, "wb") as f:
        for c in want:
            fhe.server.write_ciphertext(f, c)
    assert open(fout, "rb").read() == open(fwant, "rb").read()
    digest = sum(int(w) * (2 * i + 1) for i, w in enumerate(want.reshape(-1))) % (1 << 64)
    assert "digest=%016x" % digest in r.stdout, r.stdout
