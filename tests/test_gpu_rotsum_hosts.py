"""GPU: the hosts of the hoisted special-prime rotations on real keys (KeyGenerator.generate_special_galois_keys; RotSumPlan,
Evaluator.rotate_sum / rotate_each, circuits.packed_filter2d(fused=True), the C++ facade's seal::hip::RotSumPlan / rotate_sum_sp /
rotate_each_sp): results decrypt to what they must, the fused filter decrypts to the slots of the op-by-op filter, every call keeps the
budget circuits.rotate_sum_budget promises, and the budgets are printed beside those of the op-by-op composition."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import galois_oracle as go
import test_gpu_keyswitch_sp_hosts as kh

pytestmark = pytest.mark.gpu

N, TILE_W, PARENTS = kh.N, kh.TILE_W, kh.PARENTS
FILTERS = {"box3x3": np.ones((3, 3), dtype=np.int64), "gauss3x3": np.outer([1, 2, 1], [1, 2, 1])}


def _centred(w, t):
    w %= t
    return w - t if 2 * w > t else w


@pytest.mark.parametrize("name", list(PARENTS))
def test_rotate_sum_and_rotate_each_on_real_keys(fhe, name):
    import torch
    S = kh._setup(fhe, name)
    parent, level, ev, be, gk, t = S["parent"], S["level"], S["ev"], S["be"], S["gk"], S["level"].t
    rng = np.random.default_rng(4)
    slots = rng.integers(0, t, size=(2, N), dtype=np.uint64)
    S["enc"].seek(30)
    ct = S["enc"].encrypt_plains(be.encode(slots))
    fresh, plain = kh._exact_budgets(fhe, S, ct)
    assert np.array_equal(be.decode(plain), slots)
    moves = [(0, False), (1, False), (-1, False), (4, False), (-TILE_W, False), (0, True)]
    elts = [1 if (st, sw) == (0, False) else (2 * N - 1 if sw else fhe.galois_element(N, st)) for st, sw in moves]
    weights = [1, t - 1, (t - 1) // 2, (t + 1) // 2, 3, t - 2]
    plan = fhe.RotSumPlan(level, gk, elts, weights)
    assert plan.elements == elts and fhe.RotSumPlan(level, gk, [0, 1, -1], steps=True).elements == elts[:3]
    out = ev.rotate_sum(ct, plan)
    want = np.zeros((2, N), dtype=object)
    for (st, sw), w in zip(moves, weights):
        want = (want + w * go.permute_slots(slots.astype(object), st, sw)) % t
    after, plain = kh._exact_budgets(fhe, S, out)
    assert np.array_equal(be.decode(plain), want.astype(np.uint64))
    op = None                                                           # the op-by-op composition with the same keys
    for g, w in zip(elts, weights):
        term = ev.multiply_plain(ct if g == 1 else ev.apply_galois(ct, g, gk), np.array([w], dtype=np.uint64))
        op = term if op is None else ev.add(op, term, out=op)
    after_op, plain_op = kh._exact_budgets(fhe, S, op)
    assert np.array_equal(plain_op, plain) and not torch.equal(op, out), "the same plaintext, NOT the same ciphertext"
    lines = []
    for f, a, o in zip(fresh, after, after_op):
        bound = fhe.circuits.rotate_sum_budget(parent, f, weights)
        assert a >= bound - 1e-9, (name, f, a, bound)
        lines.append("%.2f -> fused %.2f, op-by-op %.2f (bound %.2f)" % (f, a, o, bound))
    buf = ct.clone()
    assert ev.rotate_sum(buf, plan, out=buf) is buf and torch.equal(buf, out)
    each = ev.rotate_each(ct, plan)
    assert tuple(each.shape) == (len(elts),) + tuple(ct.shape) and torch.equal(each[0], ct)
    for j, (st, sw) in enumerate(moves):
        a_each, plain = kh._exact_budgets(fhe, S, each[j])
        assert np.array_equal(be.decode(plain), go.permute_slots(slots, st, sw)), (st, sw)
        assert all(a >= fhe.circuits.special_key_switch_budget(parent, f) - 1e-9 for f, a in zip(fresh, a_each))
    print("\n[rotate_sum %s n=%d level of %d primes, %d taps, sum|w'|=%d] exact budget %s"
          % (name, N, level.k, len(elts), sum(abs(_centred(w, t)) for w in weights), "; ".join(lines)))
    with pytest.raises(ValueError, match="size 2"):
        ev.rotate_sum(level.random_ct(1, size=3), plan)
    with pytest.raises(ValueError, match="another context"):
        fhe.Evaluator(parent).rotate_sum(parent.random_ct(1), plan)
    with pytest.raises(ValueError, match="RotSumPlan expected"):
        ev.rotate_sum(ct, gk)
    with pytest.raises(ValueError, match="shape"):
        ev.rotate_sum(ct, plan, out=torch.empty_like(ct)[:1])
    with pytest.raises(ValueError, match="no special Galois key for element 7"):
        fhe.RotSumPlan(level, gk, [1, 7])
    q = list(PARENTS[name][0])
    other = fhe.SEALContext(N, [q[1], q[0]] + q[2:], t)                 # another base: its first k - 1 primes are not this level's
    okeys = fhe.KeyGenerator(other, seed=3).generate_special_galois_keys([3])
    with pytest.raises(ValueError, match="another parent"):
        fhe.RotSumPlan(level, okeys, [3])


@pytest.mark.parametrize("kind", list(FILTERS))
@pytest.mark.parametrize("name", list(PARENTS))
def test_fused_packed_filter_decrypts_to_the_op_by_op_filter(fhe, name, kind):
    S = kh._setup(fhe, name)
    parent, level, ev, be, t = S["parent"], S["level"], S["ev"], S["be"], S["level"].t
    th = N // 2 // TILE_W
    w = FILTERS[kind]
    rng = np.random.default_rng(3)
    tiles = rng.integers(0, 256, size=(2, th, TILE_W))
    S["enc"].seek(40)
    ct = S["enc"].encrypt_plains(be.encode(tiles.reshape(1, N).astype(np.uint64)))
    fresh, _ = kh._exact_budgets(fhe, S, ct)
    ref = fhe.circuits.packed_filter2d(ev, S["gk"], ct, TILE_W, w, 3, 3)
    out = fhe.circuits.packed_filter2d(ev, S["gk"], ct, TILE_W, w, 3, 3, fused=True)
    plain, budget = S["dec"].decrypt_batch(out, with_budget=True)
    plain_ref, budget_ref = S["dec"].decrypt_batch(ref, with_budget=True)
    mask = fhe.circuits.packed_filter_valid_mask(N, TILE_W, 3, 3)
    got, got_ref = be.decode(plain)[0], be.decode(plain_ref)[0]
    assert np.array_equal(got[mask], got_ref[mask])
    want = np.zeros((2, th, TILE_W), dtype=np.int64)
    for y in range(1, th - 1):
        for x in range(1, TILE_W - 1):
            want[:, y, x] = (tiles[:, y - 1:y + 2, x - 1:x + 2] * w).sum(axis=(1, 2))
    assert int(want.max()) < t and np.array_equal(got[mask], want.reshape(N)[mask].astype(np.uint64))
    bound = fhe.circuits.rotate_sum_budget(parent, min(fresh), w)
    print("\n[packed_filter2d %s %s level of %d primes] budget left: fused %r bits (bound %.2f), op-by-op %r bits" % (kind, name, level.k, budget, bound, budget_ref))
    assert min(budget) >= math.floor(bound)


def test_fused_filter_needs_every_tap_s_key(fhe):
    S = kh._setup(fhe, "P8192")
    ev, level = S["ev"], S["level"]
    ct = level.random_ct(1)
    few = S["kg"].generate_special_galois_keys([3])
    with pytest.raises(ValueError, match="no special Galois key"):
        fhe.circuits.packed_filter2d(ev, few, ct, TILE_W, FILTERS["box3x3"], 3, 3, fused=True)
    keys = S["kgl"].generate_galois_keys(30, elements=[3])
    with pytest.raises(ValueError, match="SpecialGaloisKeys expected"):
        fhe.circuits.packed_filter2d(ev, keys, ct, TILE_W, FILTERS["box3x3"], 3, 3, fused=True)
    with pytest.raises(ValueError, match="every weight is zero"):
        fhe.circuits.packed_filter2d(ev, S["gk"], ct, TILE_W, np.zeros((3, 3), dtype=np.int64), 3, 3, fused=True)


@pytest.mark.parametrize("name", list(PARENTS))
def test_cpp_host_agrees_with_the_python_host(fhe, tmp_path, name):
    """seal/rotsum_check (seal::hip::RotSumPlan, rotate_each_sp, rotate_sum_sp) on a stream of ciphertexts: the bytes of the Python host"""
    exe = os.path.join(os.path.dirname(fhe.LIB_PATH), "seal", "rotsum_check")
    assert os.path.exists(exe), "build() makes seal/rotsum_check"
    S = kh._setup(fhe, name)
    parent, level, ev, gk, t = S["parent"], S["level"], S["ev"], S["gk"], S["level"].t
    ct = level.random_ct(3, seed=78)
    elts = [1, 3, fhe.galois_element(N, -TILE_W - 1), 2 * N - 1]
    weights = [2, t - 1, (t + 1) // 2, 5]
    plan = fhe.RotSumPlan(level, gk, elts, weights)
    want = np.concatenate([fhe.to_host(ev.rotate_each(ct, plan)).reshape((-1,) + tuple(ct.shape[1:])), fhe.to_host(ev.rotate_sum(ct, plan))])
    fin, fout, fgk, ftaps, fwant = (str(tmp_path / x) for x in ("in.ct", "out.ct", "galois.keys", "taps", "want.ct"))
    with open(fin, "wb") as f:
        for c in fhe.to_host(ct):
            fhe.server.write_ciphertext(f, c)
    with open(fgk, "wb") as f:
        for g in gk.elements():
            f.write(struct.pack("<2I", g, 0))
            f.write(fhe.to_host(gk.key(g)).tobytes())
    with open(ftaps, "wb") as f:
        for g, w in zip(elts, weights):
            f.write(struct.pack("<2IQ", g, 0, w))
    with open(fwant, "wb") as f:
        for c in want:
            fhe.server.write_ciphertext(f, c)
    r = subprocess.run([exe, fin, fout, "3", fgk, ftaps, str(N), str(parent.t)] + [str(q) for q in parent.q], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(fout, "rb").read() == open(fwant, "rb").read()
    digest = sum(int(w) * (2 * i + 1) for i, w in enumerate(want.reshape(-1))) % (1 << 64)
    assert "digest=%016x" % digest in r.stdout, r.stdout
