"""GPU: the Python host of the baby-step / giant-step maps on real keys at the P8192 primes, n = 1024 (KeyGenerator.generate_special_galois_keys;
RotBsgsPlan, Evaluator.rotate_bsgs, circuits.block_matvec_bsgs, circuits.block_dct2d_matrix): the 64 x 64 matrix D (x) D of the 2-D 8 x 8 DCT
with 16 baby and 8 giant steps (22 keys) decrypts on every slot to B @ x modulo t; the measured budget is at or above
circuits.rotate_bsgs_budget; the op-by-op composition from rotate_each, multiply_plain, add and apply_galois decrypts to the same slots; the
budget of the separable pair of rotate_diag_sum calls is printed beside them; the C++ host (seal::hip::RotBsgsPlan,
rotate_bsgs_sp) writes the Python host's bytes."""
import os
import struct
import subprocess

import numpy as np
import pytest

import test_gpu_keyswitch_sp_hosts as kh

pytestmark = pytest.mark.gpu

N = kh.N
NAME = "P8192"
BABY = 16


def _op_by_op(fhe, S, ct, plan, keys):
    """rotate_each over the baby steps, per giant step the plaintext products and their sum, apply_galois, add"""
    ev = S["ev"]
    rot = ev.rotate_each(ct, fhe.RotSumPlan(S["level"], keys, plan.baby))
    out = None
    for h, row in zip(plan.giant, plan.plains):
        inner = None
        for j, p in enumerate(row):
            if not p.any():
                continue
            term = ev.multiply_plain(rot[j], p)
            inner = term if inner is None else ev.add(inner, term, out=inner)
        if h != 1:
            inner = ev.apply_galois(inner, h, keys)
        out = inner if out is None else ev.add(out, inner, out=out)
    return out


def test_block_dct2d_in_one_call(fhe):
    import torch
    S = kh._setup(fhe, NAME)
    level, ev, be, t = S["level"], S["ev"], S["be"], S["level"].t
    c = fhe.circuits
    B = c.block_dct2d_matrix(4)
    bs, gs, diags = c.block_matvec_bsgs(N, t, B, BABY)
    assert (len(bs), len(gs)) == (16, 8)
    steps = [s for s in bs + gs if s]
    keys = S["kg"].generate_special_galois_keys([fhe.galois_element(N, s) for s in steps])
    assert len(keys.elements()) == 22
    plan = fhe.RotBsgsPlan(level, keys, bs, gs, diags, steps=True)
    assert plan.baby == [fhe.galois_element(N, s) for s in bs] and plan.giant == [fhe.galois_element(N, s) for s in gs]
    rng = np.random.default_rng(64)
    x = rng.integers(0, 16, size=N)
    S["enc"].seek(60)
    ct = S["enc"].encrypt_plains(be.encode(x[None].astype(np.uint64)))
    out = ev.rotate_bsgs(ct, plan)
    fresh, _ = kh._exact_budgets(fhe, S, ct)
    after, plain = kh._exact_budgets(fhe, S, out)
    want = (np.einsum("ab,gb->ga", B.astype(object), x.reshape(N // 64, 64).astype(object)) % t).reshape(N)
    assert np.array_equal(be.decode(plain)[0], want.astype(np.uint64))
    op = _op_by_op(fhe, S, ct, plan, keys)
    after_op, plain_op = kh._exact_budgets(fhe, S, op)
    assert np.array_equal(plain_op, plain) and not torch.equal(op, out), "the same plaintext, NOT the same ciphertext"
    # the separable route: D on every row of the block (steps -7 .. 7), then D down its columns (steps -56 .. 56 in eights)
    D = c.dct8_matrix(4)
    e1, d1 = c.block_matvec_diagonals(N, t, np.kron(np.eye(8, dtype=np.int64), D))
    e2, d2 = c.block_matvec_diagonals(N, t, np.kron(D, np.eye(8, dtype=np.int64)))
    assert len(e1) == 15 and len(e2) == 15
    skeys = S["kg"].generate_special_galois_keys([g for g in e1 + e2 if g != 1])
    sep = ev.rotate_diag_sum(ev.rotate_diag_sum(ct, fhe.RotDiagPlan(level, skeys, e1, d1)), fhe.RotDiagPlan(level, skeys, e2, d2))
    after_sep, plain_sep = kh._exact_budgets(fhe, S, sep)
    assert np.array_equal(plain_sep, plain)
    for f, a, o, s in zip(fresh, after, after_op, after_sep):
        bound = c.rotate_bsgs_budget(S["parent"], f, plan.plains, plan.baby, plan.giant)
        print("\n[block_dct2d(bits=4) 16 x 8, 22 keys] exact budget %.2f -> fused %.2f, op-by-op %.2f, separable pair %.2f (bound %.2f)" % (f, a, o, s, bound))
        assert a >= bound - 1e-9, (f, a, bound)
    buf = ct.clone()
    assert ev.rotate_bsgs(buf, plan, out=buf) is buf and torch.equal(buf, out)
    with pytest.raises(ValueError, match="size 2"):
        ev.rotate_bsgs(level.random_ct(1, size=3), plan)
    with pytest.raises(ValueError, match="RotBsgsPlan expected"):
        ev.rotate_bsgs(ct, fhe.RotSumPlan(level, keys, plan.baby))
    with pytest.raises(ValueError, match="another context"):
        fhe.Evaluator(S["parent"]).rotate_bsgs(S["parent"].random_ct(1), plan)


def test_cpp_host_agrees_with_the_python_host(fhe, tmp_path):
    """seal/rotbsgs_check (seal::hip::RotBsgsPlan, rotate_bsgs_sp) on a stream of ciphertexts: the bytes of the Python host.  4 x 3 steps
    with 1 in both lists and two absent pairs"""
    exe = os.path.join(os.path.dirname(fhe.LIB_PATH), "seal", "rotbsgs_check")
    assert os.path.exists(exe), "build() makes seal/rotbsgs_check"
    S = kh._setup(fhe, NAME)
    parent, level, ev, t = S["parent"], S["level"], S["ev"], S["level"].t
    ct = level.random_ct(3, seed=81)
    bs, gs = [0, 1, 2, 3], [-4, 0, 4]
    gk = S["kg"].generate_special_galois_keys([fhe.galois_element(N, s) for s in bs + gs if s])
    rng = np.random.default_rng(12)
    diags = rng.integers(0, t, size=(3, 4, N), dtype=np.uint64)
    diags[0, 1] = 0
    diags[2, 0] = 0
    plan = fhe.RotBsgsPlan(level, gk, bs, gs, diags, steps=True)
    want = fhe.to_host(ev.rotate_bsgs(ct, plan))
    fin, fout, fgk, fplan, fwant = (str(tmp_path / x) for x in ("in.ct", "out.ct", "galois.keys", "plan", "want.ct"))
    with open(fin, "wb") as f:
        for c in fhe.to_host(ct):
            fhe.server.write_ciphertext(f, c)
    with open(fgk, "wb") as f:
        for g in gk.elements():
            f.write(struct.pack("<2I", g, 0))
            f.write(fhe.to_host(gk.key(g)).tobytes())
    with open(fplan, "wb") as f:
        f.write(struct.pack("<2I", len(plan.baby), len(plan.giant)))
        f.write(np.array(plan.baby, dtype=np.uint32).tobytes())
        f.write(np.array(plan.giant, dtype=np.uint32).tobytes())
        f.write(np.ascontiguousarray(diags, dtype=np.uint64).tobytes())
    with open(fwant, "wb") as f:
        for c in want:
            fhe.server.write_ciphertext(f, c)
    r = subprocess.run([exe, fin, fout, "3", fgk, fplan, str(N), str(parent.t)] + [str(q) for q in parent.q], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(fout, "rb").read() == open(fwant, "rb").read()
    digest = sum(int(w) * (2 * i + 1) for i, w in enumerate(want.reshape(-1))) % (1 << 64)
    assert "digest=%016x" % digest in r.stdout, r.stdout
