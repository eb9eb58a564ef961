"""GPU: the hosts of the diagonal linear maps on real keys at the P8192 primes (KeyGenerator.generate_special_galois_keys; RotDiagPlan,
Evaluator.rotate_diag_sum, circuits.packed_filter2d(border=...), circuits.block_matvec_diagonals, the C++ facade's seal::hip::RotDiagPlan /
rotate_diag_sum_sp): every slot decrypts to the numpy model, the border included; the measured budget is at or above
circuits.rotate_diag_budget and within a bit of the op-by-op composition's; the C++ host writes the Python host's bytes."""
import os
import struct
import subprocess

import numpy as np
import pytest

import test_gpu_keyswitch_sp_hosts as kh

pytestmark = pytest.mark.gpu

N, TILE_W = kh.N, kh.TILE_W
NAME = "P8192"
BOX = np.ones((3, 3), dtype=np.int64)
_keys = {}


def _op_by_op(fhe, S, ct, plan, keys):
    """rotate, multiply_plain by the encoded diagonal, add: the composition the fused call stands for"""
    ev, op = S["ev"], None
    for g, p in zip(plan.elements, plan.plains):
        term = ev.multiply_plain(ct if g == 1 else ev.apply_galois(ct, g, keys), p)
        op = term if op is None else ev.add(op, term, out=op)
    return op


def _check_budget(fhe, S, ct, out, plan, keys, what):
    import torch
    fresh, _ = kh._exact_budgets(fhe, S, ct)
    after, plain = kh._exact_budgets(fhe, S, out)
    op = _op_by_op(fhe, S, ct, plan, keys)
    after_op, plain_op = kh._exact_budgets(fhe, S, op)
    assert np.array_equal(plain_op, plain) and not torch.equal(op, out), "the same plaintext, NOT the same ciphertext"
    for f, a, o in zip(fresh, after, after_op):
        bound = fhe.circuits.rotate_diag_budget(S["parent"], f, plan.plains)
        print("\n[%s] exact budget %.2f -> fused %.2f, op-by-op %.2f (bound %.2f)" % (what, f, a, o, bound))
        assert a >= bound - 1e-9, (what, f, a, bound)
        assert abs(a - o) <= 1.0, (what, "not within a bit of the op-by-op composition", a, o)
    return plain


@pytest.mark.parametrize("border", ["zero", "clamp"])
def test_bordered_packed_filter_decrypts_on_every_slot(fhe, border):
    S = kh._setup(fhe, NAME)
    level, ev, be, gk, t = S["level"], S["ev"], S["be"], S["gk"], S["level"].t
    c = fhe.circuits
    th = N // 2 // TILE_W
    rng = np.random.default_rng(3)
    tiles = rng.integers(0, 256, size=(2, th, TILE_W))
    S["enc"].seek(40)
    ct = S["enc"].encrypt_plains(be.encode(tiles.reshape(1, N).astype(np.uint64)))
    out = c.packed_filter2d(ev, gk, ct, TILE_W, BOX, 3, 3, border=border)
    plan = next(p for tag, p in gk.plans.items() if len(tag) > 2 and tag[1] == "diag" and tag[2] == border)
    assert c.packed_filter2d(ev, gk, ct, TILE_W, BOX, 3, 3, border=border) is not out and sum(1 for tag in gk.plans if tag[1:3] == ("diag", border)) == 1
    plain = _check_budget(fhe, S, ct, out, plan, gk, "packed_filter2d box3x3 border=%s" % border)
    got = be.decode(plain)[0]
    want = np.stack([c.packed_filter_border_model(tiles[r], BOX, 3, 3, t, None, border) for r in range(2)]).reshape(N).astype(np.uint64)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    mask = c.packed_filter_valid_mask(N, TILE_W, 3, 3)
    fused = be.decode(S["dec"].decrypt_batch(c.packed_filter2d(ev, gk, ct, TILE_W, BOX, 3, 3, fused=True)))[0]
    assert np.array_equal(got[mask], fused[mask]) and not np.array_equal(got[~mask], fused[~mask])
    few = S["kg"].generate_special_galois_keys([3])
    with pytest.raises(ValueError, match="no special Galois key"):
        c.packed_filter2d(ev, few, ct, TILE_W, BOX, 3, 3, border=border)


def _matvec_keys(fhe, S, d):
    if d not in _keys:
        _keys[d] = S["kg"].generate_special_galois_keys([fhe.galois_element(N, s) for s in range(-(d - 1), d) if s])
    return _keys[d]


def test_block_matvec_with_the_dct8_matrix(fhe):
    S = kh._setup(fhe, NAME)
    level, ev, be, t = S["level"], S["ev"], S["be"], S["level"].t
    B = fhe.circuits.dct8_matrix(bits=4)
    elts, diags = fhe.circuits.block_matvec_diagonals(N, t, B)
    keys = _matvec_keys(fhe, S, 8)
    plan = fhe.RotDiagPlan(level, keys, elts, diags)
    assert fhe.RotDiagPlan(level, keys, list(range(-7, 8)), diags, steps=True).elements == elts
    rng = np.random.default_rng(8)
    x = rng.integers(0, 16, size=N)
    S["enc"].seek(50)
    ct = S["enc"].encrypt_plains(be.encode(x[None].astype(np.uint64)))
    out = ev.rotate_diag_sum(ct, plan)
    plain = _check_budget(fhe, S, ct, out, plan, keys, "block_matvec dct8(bits=4)")
    want = (np.einsum("ab,gb->ga", B.astype(object), x.reshape(N // 8, 8).astype(object)) % t).reshape(N)
    assert np.array_equal(be.decode(plain)[0], want.astype(np.uint64))
    import torch
    buf = ct.clone()
    assert ev.rotate_diag_sum(buf, plan, out=buf) is buf and torch.equal(buf, out)
    with pytest.raises(ValueError, match="size 2"):
        ev.rotate_diag_sum(level.random_ct(1, size=3), plan)
    with pytest.raises(ValueError, match="RotDiagPlan expected"):
        ev.rotate_diag_sum(ct, fhe.RotSumPlan(level, keys, elts))
    with pytest.raises(ValueError, match="another context"):
        fhe.Evaluator(S["parent"]).rotate_diag_sum(S["parent"].random_ct(1), plan)


def test_cpp_host_agrees_with_the_python_host(fhe, tmp_path):
    """seal/rotdiag_check (seal::hip::RotDiagPlan, rotate_diag_sum_sp) on a stream of ciphertexts: the bytes of the Python host"""
    exe = os.path.join(os.path.dirname(fhe.LIB_PATH), "seal", "rotdiag_check")
    assert os.path.exists(exe), "build() makes seal/rotdiag_check"
    S = kh._setup(fhe, NAME)
    parent, level, ev, gk, t = S["parent"], S["level"], S["ev"], S["gk"], S["level"].t
    ct = level.random_ct(3, seed=79)
    elts, diags = fhe.circuits.packed_filter_diagonals(N, t, TILE_W, [1, 2, 1, 2, 4, 2, 1, 2, t - 1], 3, 3, border="clamp")
    plan = fhe.RotDiagPlan(level, gk, elts, diags)
    want = fhe.to_host(ev.rotate_diag_sum(ct, plan))
    fin, fout, fgk, ftaps, fwant = (str(tmp_path / x) for x in ("in.ct", "out.ct", "galois.keys", "taps", "want.ct"))
    with open(fin, "wb") as f:
        for c in fhe.to_host(ct):
            fhe.server.write_ciphertext(f, c)
    with open(fgk, "wb") as f:
        for g in gk.elements():
            f.write(struct.pack("<2I", g, 0))
            f.write(fhe.to_host(gk.key(g)).tobytes())
    with open(ftaps, "wb") as f:
        for g, d in zip(elts, diags):
            f.write(struct.pack("<2I", g, 0))
            f.write(np.ascontiguousarray(d, dtype=np.uint64).tobytes())
    with open(fwant, "wb") as f:
        for c in want:
            fhe.server.write_ciphertext(f, c)
    r = subprocess.run([exe, fin, fout, "3", fgk, ftaps, str(N), str(parent.t)] + [str(q) for q in parent.q], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(fout, "rb").read() == open(fwant, "rb").read()
    digest = sum(int(w) * (2 * i + 1) for i, w in enumerate(want.reshape(-1))) % (1 << 64)
    assert "digest=%016x" % digest in r.stdout, r.stdout
